#!/usr/bin/env python3
"""Golden vectors of Urgency-Pair, MLP-Pair and MLP-ContextPair at the reference's scaled token pads (max_tasks = 64, max_agents = 48), by
RUNNING the reference (builder's container only; data only is written).

    python tools/gen_golden_wide_pads.py [traces] [metrics] [pair_traces] [pair_metrics] [ctx_traces] [ctx_metrics] [--probe-tasks]

UrgencyPair(max_tasks=64, max_agents=48) (TaskAllocation/Hybrid/PairCostHybrid.py:31-86,520-550) as experiments/wps_eval.py:422-434
builds it for the WPS_attn_L / _XL / _OS18 / _OS24 / WPS_scale / WPS_oversized suites, driven by the harness loop
(experiments/wps_eval.py:248-254: _should_replan with interval 15) over the reference env built as tools/gen_golden.py builds it.
Output under tests/golden/:

  urgpair48_trace_<case>_s0.npz   one episode.  The fields of urgpair_trace_* (metrics, n_replans, actions, lsap_step, lsap_shape) and
                                  per plan: step, scores [48, 64] float32 (urgency_edge_scores), ev (edge_valid), tid / aid (token
                                  column / row ids, -1 = pad), selected (PairCostHybrid._selected_mask's rule), pairs (step, agent id,
                                  task id); per step replanned; n_live / n_under per plan (live agents, underfilled tasks in front of
                                  the truncation) and their maxima; the spec overrides the case was derived with (tasks_att / tasks_rec
                                  and the tile, 0 = the registry's).  With these the trace replays through allocate_scored.
                                  The LSAP cost matrices are left out: 40 x 64 doubles per round outgrow the fixture size.
  urgpair48_metrics_<case>.npz    8 seeds: the 30 metrics and hung.n_replans

The learned kinds: PairCostHybrid(use_attention=False, max_tasks=64, max_agents=48) and the matching ContextPairHybrid, with the weight
sets tools/gen_golden_mlp_pair.py / gen_golden_mlp_context_pair.py wrote (an MLP's weights do not depend on the pads), through those
files' own episode loops with their two pad-dependent names (new_policy, _ids) bound to the wide pads here:

  mlppair48_trace_<tag>_s<seed>.npz, mlpctx48_trace_<tag>_s<seed>.npz      the formats of mlppair_trace_* / mlpctx_trace_* at [48, 64]
  mlppair48_metrics_<case>.npz, mlpctx48_metrics_<case>.npz               metrics32 / metrics64 per seed (init2, interval 15), `seeds`
Each metrics run records seeds 0-15 of the three cases and ends on the condition the issue set for the episode test, per kind: E >= 48
episodes over >= 3 cases and F_ref (episodes whose float32-score and float64-score runs of the reference differ) <= E / 10.  MLP-Pair:
F_ref = 3 of 48 (seeds OS24 / 0, L / 6, XL / 5): holds.  MLP-ContextPair: F_ref = 5 of 48 (L / 0, 3, 6; XL / 0, 1), and extending the seed
range does not bring it under E / 10 (9 of 72, 13 of 96, 15 of 120, 19 of 144, 20 of 168, 22 of 192 with 64 seeds per case): its run ends on
the failed assertion AFTER writing the files — both columns are the reference's own results — and the episode test of that kind applies its
rule, at most E / 10 + F_ref episodes equal to neither column, with the F_ref the files hold.

<case> = a registry case, or WPS_burst64_T<att>x<rec>: WPS_burst64 with tasks={"Att": att, "Rec": rec} — the configuration whose
plans see more than 64 underfilled tasks, so that the task truncation is exercised (WPS_burst64 itself exercises the agent
truncation: 64 live agents, at most 50 underfilled tasks).  --probe-tasks prints the maximum for a few task counts.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_golden import CASE_SPECS, HA, METRIC_KEYS, OUT, WPS_ENV_FLAGS, LsapTap, MultiUAVEnv, _events, _ids, linear_sum_assignment, make_config  # noqa: E402  (installs refshim)

from experiments.wps_eval import _apply_assign, _should_replan  # noqa: E402
from TaskAllocation.Hybrid.PairCostHybrid import PairCostHybrid, UrgencyPair  # noqa: E402

MT, MA = 64, 48
BURST_TASKS = (36, 72)  # tasks={"Att": 36, "Rec": 72} on WPS_burst64: 110 / 75 / 72 underfilled tasks at the first three plans of seed 0 (24 x 48: 74 at the first
#                         only; 20 x 40: never above 62) while the episode holds at most 110 task ids at once, within the 128 slots of the tile; see --probe-tasks
CASES = ["WPS_attn_OS24", "WPS_attn_L", "WPS_attn_XL", "WPS_burst64", "WPS_burst64_T%dx%d" % BURST_TASKS]
METRIC_CASES = ["WPS_attn_OS24", "WPS_attn_L", "WPS_attn_XL"]


def spec_of(case):
    """(spec dict, tasks_att, tasks_rec): a registry case or WPS_burst64_T<att>x<rec>"""
    if case in CASE_SPECS:
        return CASE_SPECS[case], 0, 0
    base, _, tail = case.rpartition("_T")
    att, rec = (int(x) for x in tail.split("x"))
    spec = dict(CASE_SPECS[base])
    spec["tasks"] = {"Att": att, "Rec": rec, "Hold": 0}
    return spec, att, rec


def make_env(case):
    cfg = make_config(spec_of(case)[0], dict(WPS_ENV_FLAGS))
    cfg.multiple_tasks_per_agent = True
    return MultiUAVEnv(cfg)


def selected_mask(tok, result):
    """UrgencyPair has no _selected_mask of its own: the reference's PairCostHybrid._selected_mask is called on the plan's tokens and result"""
    return PairCostHybrid._selected_mask(types.SimpleNamespace(max_agents=MA, max_tasks=MT), tok, result)


def n_underfilled(env):
    """build_att_tokens' open_tasks in front of the [:max_tasks] cut (AttentionRAH.py:69-73)"""
    n = 0
    for t in env.tasks:
        if getattr(t, "status", 0) == 2:
            continue
        if float(t.allocatedReqs[t.typeIdx]) < float(t.currentReqs[t.typeIdx]):
            n += 1
    return n


def run_episode(case, seed, record):
    env = make_env(case)
    tap = LsapTap()
    HA.linear_sum_assignment = tap
    try:
        obs, info = env.reset(seed=seed)
        hung = HA.HungarianAllocator(replan_interval=20, max_coord=env.max_coord)
        urg = UrgencyPair(max_tasks=MT, max_agents=MA)
        done = {a: False for a in env.agents}
        trunc = {a: False for a in env.agents}
        rec = {k: [] for k in ("step", "scores", "ev", "tid", "aid", "selected", "n_live", "n_under")}
        pairs, acts, replanned, latest = [], [], [], None
        while not all(done.values()) and not all(trunc.values()):
            events = _events(info)
            actions = {}
            tap.step = env.time_steps
            rp = bool(_should_replan(env, events))
            replanned.append(int(rp))
            if rp:
                n_under = n_underfilled(env)
                result, tok, scores = urg.plan(env, hung, events=events, force=True)
                actions = _apply_assign(env, result)
                assert len(tok["open_tasks"]) == min(n_under, MT), (len(tok["open_tasks"]), n_under)
                tid, aid = _ids(tok, MT, MA)
                for k, v in zip(rec, (env.time_steps, scores, tok["edge_valid"], tid, aid, selected_mask(tok, result), len(tok["live"]), n_under)):
                    rec[k].append(np.asarray(v).copy())
                for name, task in result:
                    pairs.append((env.time_steps, env.agent_by_name[name].id, task.id))
                for name, idx in actions.items():
                    acts.append((env.time_steps, env.agent_by_name[name].id, env.last_tasks_info[idx].id, idx))
            obs, reward, done, trunc, info = env.step(actions)
            if "metrics" in info:
                latest = info["metrics"]
    finally:
        HA.linear_sum_assignment = linear_sum_assignment
    out = {"metrics": np.array([float(latest[k]) for k in METRIC_KEYS]), "n_replans": np.int64(hung.n_replans)}
    if record:
        out.update({k: np.stack(v) for k, v in rec.items()})
        out.update(pairs=np.array(pairs, dtype=np.int64).reshape(-1, 3), actions=np.array(acts, dtype=np.int64).reshape(-1, 4),
                   replanned=np.array(replanned, dtype=np.int64), lsap_step=np.array([c[0] for c in tap.calls], dtype=np.int64),
                   lsap_shape=np.array([c[1].shape for c in tap.calls], dtype=np.int64).reshape(-1, 2),
                   n_live_max=np.int64(max(rec["n_live"])), n_under_max=np.int64(max(rec["n_under"])))
    return out


def gen_traces():
    for case in CASES:
        _, att, rec = spec_of(case)
        tr = run_episode(case, 0, True)
        tr.update(case=np.array(case), seed=np.int64(0), interval=np.int64(15), max_tasks=np.int64(MT), max_agents=np.int64(MA),
                  tasks_att=np.int64(att), tasks_rec=np.int64(rec), keys=np.array(METRIC_KEYS))
        path = os.path.join(OUT, f"urgpair48_trace_{case}_s0.npz")
        np.savez_compressed(path, **tr)
        ev = tr["ev"] != 0
        print(path, os.path.getsize(path), "B  plans", len(tr["step"]), "valid share", float(ev.mean()), "rows >= 16 valid", int(ev[:, 16:].sum()),
              "cols >= 32 valid", int(ev[:, :, 32:].sum()), "n_live_max", int(tr["n_live_max"]), "n_under_max", int(tr["n_under_max"]),
              "S_WPS", tr["metrics"][4], "replans", int(tr["n_replans"]), flush=True)
    g = np.load(os.path.join(OUT, f"urgpair48_trace_{CASES[-1]}_s0.npz"))
    assert int(g["n_under_max"]) > MT and int(g["n_live_max"]) > MA, "the truncation case does not truncate"


def gen_metrics():
    for case in METRIC_CASES:
        rows, reps = [], []
        for s in range(8):
            r = run_episode(case, s, False)
            rows.append(r["metrics"]); reps.append(int(r["n_replans"]))
        path = os.path.join(OUT, f"urgpair48_metrics_{case}.npz")
        np.savez_compressed(path, metrics=np.stack(rows), n_replans=np.array(reps, dtype=np.int64), keys=np.array(METRIC_KEYS), case=np.array(case),
                            max_tasks=np.int64(MT), max_agents=np.int64(MA))
        print(path, "mean S_WPS", np.stack(rows)[:, 4].mean(), flush=True)


def probe_tasks():
    for att, rec in ((20, 40), (24, 48), (28, 56), (32, 64), (36, 72)):
        tr = run_episode(f"WPS_burst64_T{att}x{rec}", 0, True)
        print("tasks", att, rec, "n_under per plan", tr["n_under"].tolist(), "n_live_max", int(tr["n_live_max"]), flush=True)


# ---- the learned kinds ---------------------------------------------------------------------------------------------------------------
LEARNED_TRACES = {"pair": [("WPS_attn_OS24", "init2", 15, 0), ("WPS_attn_L", "init2", 15, 0), ("WPS_attn_XL", "init2", 15, 0), ("WPS_attn_L", "init2_raw", 20, 0)],
                  "ctx": [("WPS_attn_XL", "init2", 15, 0), ("WPS_attn_OS24", "init2", 15, 0)]}
LEARNED_CAP = 400 * 1024  # bytes per fixture, as the tests of the narrow fixtures require


def learned(kind):
    """the narrow generator's module with its pad-dependent names bound to 64 x 48, and the fixture prefix"""
    if kind == "pair":
        import gen_golden_mlp_pair as G
        from TaskAllocation.Hybrid.PairCostHybrid import PairCostHybrid as Hybrid
        prefix = "mlppair48"
    else:
        import gen_golden_mlp_context_pair as G
        from TaskAllocation.Hybrid.ContextPairHybrid import ContextPairHybrid as Hybrid
        prefix = "mlpctx48"
    G.new_policy = lambda raw: Hybrid(use_attention=False, max_tasks=MT, max_agents=MA, raw_features=raw, device="cpu")
    G._ids = lambda tok, mt, ma: _ids(tok, MT, MA)
    return G, prefix


PER_PLAN = ("step", "tf", "af", "tid", "aid", "tmask", "amask", "ev", "ctx", "scores", "logits", "scores64", "selected")


def gen_learned_traces(kind):
    G, prefix = learned(kind)
    for case, wset, interval, seed in LEARNED_TRACES[kind]:
        policy, w = G.load_policy(wset)
        tr = G.run_episode(case, seed, policy, w, interval, False, True)
        ev = tr["ev"] != 0
        d_ref = float(np.abs(tr["scores"].astype(np.float64) - tr["scores64"])[ev].max())
        n_all = len(tr["step"])
        tr.update(case=np.array(case), weights=np.array(wset), interval=np.int64(interval), seed=np.int64(seed), d_ref=np.float64(d_ref),
                  max_tasks=np.int64(MT), max_agents=np.int64(MA), n_plans=np.int64(n_all))
        path = os.path.join(OUT, f"{prefix}_trace_{G.tag_of(case, wset, interval)}_s{seed}.npz")
        keep = n_all
        while True:  # (a trace that outgrows the cap keeps its first `keep` plans in full; pairs / actions / replanned stay whole)
            out = {k: (v[:keep] if k in PER_PLAN else v) for k, v in tr.items()}
            np.savez_compressed(path, **out)
            if os.path.getsize(path) <= LEARNED_CAP:
                break
            keep -= 2
        print(path, os.path.getsize(path), "B  plans", n_all, "in full", keep, "valid share", float(ev.mean()), "rows >= 16 valid", int(ev[:, 16:].sum()),
              "cols >= 32 valid", int(ev[:, :, 32:].sum()), "logit span", float(tr["logits"][ev].min()), float(tr["logits"][ev].max()), "D_ref", d_ref,
              "S_WPS", tr["metrics"][4], "replans", int(tr["n_replans"]), int(tr["policy_n_replans"]), flush=True)


def gen_learned_metrics(kind):
    G, prefix = learned(kind)
    policy, w = G.load_policy("init2")
    cols = {case: {k: [] for k in ("metrics32", "n_replans32", "policy_n_replans32", "metrics64", "n_replans64", "seeds")} for case in METRIC_CASES}
    for case in METRIC_CASES:
        c = cols[case]
        for s in range(16):
            a = G.run_episode(case, s, policy, w, 15, False, False)
            b = G.run_episode(case, s, policy, w, 15, True, False)
            c["metrics32"].append(a["metrics"]); c["n_replans32"].append(int(a["n_replans"])); c["policy_n_replans32"].append(int(a["policy_n_replans"]))
            c["metrics64"].append(b["metrics"]); c["n_replans64"].append(int(b["n_replans"])); c["seeds"].append(s)
            print(prefix, case, s, "S_WPS", a["metrics"][4], b["metrics"][4], flush=True)
    E = F = 0
    for case in METRIC_CASES:
        c = cols[case]
        differ = [not (np.array_equal(x, y) and ra == rb) for x, y, ra, rb in zip(c["metrics32"], c["metrics64"], c["n_replans32"], c["n_replans64"])]
        E += len(differ); F += sum(differ)
        print(prefix, case, "F_ref", sum(differ), "of", len(differ), "seeds", [s for s, d in zip(c["seeds"], differ) if d], flush=True)
        np.savez_compressed(os.path.join(OUT, f"{prefix}_metrics_{case}.npz"), metrics32=np.stack(c["metrics32"]), metrics64=np.stack(c["metrics64"]),
                            n_replans32=np.array(c["n_replans32"], dtype=np.int64), n_replans64=np.array(c["n_replans64"], dtype=np.int64),
                            policy_n_replans32=np.array(c["policy_n_replans32"], dtype=np.int64), seeds=np.array(c["seeds"], dtype=np.int64),
                            case=np.array(case), weights=np.array("init2"), interval=np.int64(15), keys=np.array(METRIC_KEYS),
                            max_tasks=np.int64(MT), max_agents=np.int64(MA))
    print(f"condition of the episode test ({prefix}): E = {E} over {len(METRIC_CASES)} cases, F_ref = {F}", flush=True)
    # (the two columns are the reference's results whatever F_ref is and are written above; the condition is what the run ends on)
    assert E >= 48 and len(METRIC_CASES) >= 3 and F * 10 <= E, "the fixtures do not meet E >= 48 over >= 3 cases with F_ref <= E / 10"


def main():
    if "--probe-tasks" in sys.argv:
        return probe_tasks()
    what = [a for a in sys.argv[1:]] or ["traces", "metrics", "pair_traces", "pair_metrics", "ctx_traces", "ctx_metrics"]
    if "traces" in what:
        gen_traces()
    if "metrics" in what:
        gen_metrics()
    for kind in ("pair", "ctx"):
        if f"{kind}_traces" in what:
            gen_learned_traces(kind)
        if f"{kind}_metrics" in what:
            gen_learned_metrics(kind)


if __name__ == "__main__":
    main()
