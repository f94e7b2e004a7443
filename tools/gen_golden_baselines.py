#!/usr/bin/env python3
"""Golden vectors of the two classical baselines, by RUNNING the reference (builder's container only; data only is written).

    python tools/gen_golden_baselines.py [pi|capgreedy] [case ...]

Local-PI (TaskAllocation/MarketBased/PerformanceImpact.py) and Local-Cap-Greedy (TaskAllocation/BehaviourBased/CapabilityGreedy.py)
driven with the evaluation harness's own loop (experiments/wps_eval.py:147-167; the escort cases as experiments/escort_eval.py
:162-175, replan interval 12) over the reference env built as tools/gen_golden.py builds it (make_env: the project's scenario
registry, which also holds WPS_hard_x2 / WPS_burst64).  Output under tests/golden/:

  pi_trace_<case>_s<seed>.npz / capgreedy_trace_<case>_s<seed>.npz   actions [(t, agent id, task id, index)], n_replans, metrics
  pi_metrics_<case>.npz / capgreedy_metrics_<case>.npz             seeds 0..N-1 x 30 metrics, n_replans per seed

n_replans is the allocator's own counter (PerformanceImpact.n_replans: every plan its gate let through); 0 for Cap-Greedy.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_golden import METRIC_KEYS, OUT, make_env  # noqa: E402  (installs refshim)

from experiments.paper_eval import _events, _open_tasks  # noqa: E402
from experiments.wps_eval import _apply_assign  # noqa: E402
from TaskAllocation.BehaviourBased.CapabilityGreedy import CapabilityGreedy  # noqa: E402
from TaskAllocation.MarketBased.PerformanceImpact import PerformanceImpact  # noqa: E402

# case, replan interval, seeds with a trace, metric seeds
PI_PLAN = [("WPS_hard", 20, (0, 1), 32), ("WPS_attn", 20, (0,), 32), ("WPS_hard_x2", 20, (0,), 32),
           ("WPS_escort", 12, (0, 1), 32), ("WPS_escort24", 12, (0,), 16), ("WPS_burst64", 20, (0,), 16)]
CG_PLAN = [("WPS_hard", 20, (0,), 32), ("WPS_attn", 20, (0,), 32), ("WPS_hard_x2", 20, (0,), 32), ("WPS_burst64", 20, (0,), 16)]


def run_episode(algo, case, seed, interval):
    env = make_env(case)
    obs, info = env.reset(seed=seed)
    pi = PerformanceImpact(max_coord=env.max_coord, seed=seed, replan_interval=interval)
    cap_g = CapabilityGreedy()
    done = {a: False for a in env.agents}
    trunc = {a: False for a in env.agents}
    rows, latest = [], None
    while not all(done.values()) and not all(trunc.values()):
        events = _events(info)
        actions = {}
        if algo == "pi":  # wps_eval.py:147-159 (escort_eval.py:162-175 is the same call)
            result = pi.allocate_tasks(env.get_live_agents(), _open_tasks(env), time_step=env.time_steps, events=events,
                                       agent_known_ids=env.agent_visibility_map(), max_tasks_per_agent=1)
            actions = _apply_assign(env, result)
        else:  # wps_eval.py:160-167
            vis = env.agent_visibility_map()
            act = cap_g.allocate_tasks(env.get_live_agents(), _open_tasks(env))
            if act and env.last_tasks_info and act[0][1] in env.last_tasks_info:
                agent_name, task = act[0][0], act[0][1]
                if vis is None or task.id in vis.get(agent_name, set()):
                    actions[agent_name] = env.last_tasks_info.index(task)
        for name, idx in actions.items():
            rows.append((env.time_steps, env.agent_by_name[name].id, env.last_tasks_info[idx].id, idx))
        obs, reward, done, trunc, info = env.step(actions)
        if isinstance(info, dict) and "metrics" in info:
            latest = info["metrics"]
    return {"metrics": np.array([float(latest[k]) for k in METRIC_KEYS]), "n_replans": np.int64(pi.n_replans if algo == "pi" else 0),
            "actions": np.array(rows, dtype=np.int64).reshape(-1, 4), "interval": np.int64(interval), "seed": np.int64(seed)}


def main():
    algos = [a for a in ("pi", "capgreedy") if a in sys.argv[1:]] or ["pi", "capgreedy"]
    only = [c for c in sys.argv[1:] if c not in ("pi", "capgreedy")]
    for algo in algos:
        for case, interval, trace_seeds, n_metric in (PI_PLAN if algo == "pi" else CG_PLAN):
            if only and case not in only:
                continue
            for s in trace_seeds:
                tr = run_episode(algo, case, s, interval)
                path = os.path.join(OUT, f"{algo}_trace_{case}_s{s}.npz")
                np.savez_compressed(path, **tr)
                print(path, os.path.getsize(path), "B  S_WPS", tr["metrics"][4], "replans", int(tr["n_replans"]), flush=True)
            rows, reps = [], []
            for s in range(n_metric):
                r = run_episode(algo, case, s, interval)
                rows.append(r["metrics"]); reps.append(int(r["n_replans"]))
            path = os.path.join(OUT, f"{algo}_metrics_{case}.npz")
            np.savez_compressed(path, metrics=np.stack(rows), n_replans=np.array(reps, dtype=np.int64), interval=np.int64(interval),
                                keys=np.array(METRIC_KEYS))
            print(path, "mean S_WPS", np.stack(rows)[:, 4].mean(), flush=True)


if __name__ == "__main__":
    main()
