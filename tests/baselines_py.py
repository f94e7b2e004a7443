"""Host restatement of the two classical baselines the device runs as MUAVTA_ALLOC_CAP_GREEDY / MUAVTA_ALLOC_PI, written from their
semantics (not copied), over the reference's object model: anything with the attributes of MultiUAVEnv / UAV / Task works — the
facade's object views (muavta_amd.env.MultiUAVEnv on any backend) or, where the checkout is importable, the reference env itself.
The oracle (oracle/) is frozen and does not know these modes; this module is the CPU yardstick the GPU tests compare against.

  CapGreedy   TaskAllocation/BehaviourBased/CapabilityGreedy.py:14-47, driven as experiments/wps_eval.py:160-167
  PI          TaskAllocation/MarketBased/PerformanceImpact.py:49-166 with max_tasks_per_agent=1 (slots / eligibility of
              TaskAllocation/MarketBased/CBBA.py:10-65), driven as wps_eval.py:147-159 / escort_eval.py:162-175
"""
from __future__ import annotations

import math

import numpy as np

# every tag the env emits (PerformanceImpact.py:18-24)
REPLAN_EVENTS = ("Reset_Allocation", "New_Threat", "Agent_Fail", "Escort_Created", "Escort_Retired")


def is_coalition(task) -> bool:  # CBBA.py:10-14
    return getattr(task, "kind", None) == "Escort" or float(getattr(task, "required_agents", 0) or 0) > 0


def residual(task) -> float:  # CBBA.py:17-25 == paper_eval._task_residual
    if is_coalition(task):
        need = float(getattr(task, "required_agents", 1) or 1)
        return max(need - len(getattr(task, "allocationDetails", {}) or {}), 0.0)
    return max(float(task.currentReqs[task.typeIdx] - task.allocatedReqs[task.typeIdx]), 0.0)


def open_tasks(env):  # experiments/paper_eval.py:96-101
    return [t for t in env.tasks if t.id != 0 and t.status != 2 and residual(t) > 0]


def events_of(info):  # experiments/paper_eval.py:103-106
    return list(info.get("events") or []) if isinstance(info, dict) else []


def cap_greedy_pick(live, tasks):
    """The one (agent, task) pair CapabilityGreedy returns, or None: over live agents x tasks with allocatedReqs < currentReqs at the
    type index, skipping cap <= 1e-6 and missing <= 0, the first strict maximum of min(cap, missing) * 10 - |dp| / 1000."""
    cands = [t for t in tasks if t.id != 0 and t.status != 2 and t.allocatedReqs[t.typeIdx] < t.currentReqs[t.typeIdx]]
    top, pick = -math.inf, None
    for ag in live:
        for t in cands:
            c = float(ag.currentCap2Task[t.typeIdx])
            if c <= 1e-6:
                continue
            short = max(float(t.currentReqs[t.typeIdx] - t.allocatedReqs[t.typeIdx]), 0.0)
            if short <= 0:
                continue
            d = float(np.linalg.norm(ag.position - t.position))
            val = min(c, short) * 10.0 - d / 1000.0
            if val > top:
                top, pick = val, (ag, t)
    return pick


def cap_greedy_actions(env, use_visibility=True):
    """wps_eval.py:160-167: the pick is applied only if its task is in last_tasks_info and known to the agent."""
    live = [a for a in env.get_live_agents() if getattr(a, "state", 0) != -1]
    pick = cap_greedy_pick(live, open_tasks(env))
    vis = env.agent_visibility_map() if use_visibility else None
    if pick is None or not env.last_tasks_info or pick[1] not in env.last_tasks_info:
        return {}
    ag, t = pick
    if vis is not None and t.id not in vis.get(ag.name, set()):
        return {}
    return {ag.name: env.last_tasks_info.index(t)}


class PI:
    """PerformanceImpact with one task per agent.  A path is then empty or one slot long, and for agent a and task t
    ipi == provisional rpi == rpi == cost(a, t) (with base cost 0.0), so the inclusion loop reduces to the tuple-ordered choice below.
    The consensus pass (:168-223) has nothing to resolve then: a steal removes the slot from its loser, so no slot has two claimants,
    and the winner's schedule was found feasible at the same time step.  tests/test_baselines_cpu.py confirms it by comparing this
    class with the reference's own allocate_tasks (consensus pass included) step by step."""

    def __init__(self, replan_interval=20):
        self.interval = max(1, int(replan_interval))
        self.last_plan_step = -10**9
        self.n_replans = 0
        self.n_calls = 0

    def gate(self, t, events):  # should_replan (:49-57)
        if t - self.last_plan_step >= self.interval:
            return True
        return any((ev[0] if isinstance(ev, (list, tuple)) and ev else ev) in REPLAN_EVENTS for ev in events or [])

    @staticmethod
    def slots(tasks):  # expand_slot_keys (CBBA.py:47-65): (key, task) in task order
        out = []
        for t in tasks:
            if t.id == 0 or t.status == 2:
                continue
            r = residual(t)
            if r <= 0:
                continue
            if is_coalition(t):
                out += [(f"{t.id}#c{k}", t) for k in range(int(np.ceil(r)))]
            else:
                out += [(f"{t.id}#r{k}", t) for k in range(max(1, int(np.ceil(min(r, 4.0)))))]
        return out

    @staticmethod
    def eligible(ag, t, known):  # agent_eligible (CBBA.py:28-44)
        if getattr(ag, "state", 0) == -1 or (known is not None and t.id not in known):
            return False
        el = getattr(t, "eligible_agent_types", None)
        if el is not None and getattr(ag, "type", None) not in ({el} if isinstance(el, str) else el):
            return False
        if ag.id in (getattr(t, "allocationDetails", {}) or {}):
            return False
        return True if is_coalition(t) else float(ag.currentCap2Task[t.typeIdx]) > 0

    @staticmethod
    def cost(ag, t, now):
        """_path_cost([slot of t]) for an agent with an empty path, or inf where the start misses hard_deadline by more than 1e-6."""
        t0 = max(float(getattr(ag, "next_free_time", 0) or 0), float(now))
        v = max(float(getattr(ag, "max_speed", 1.0) or 1.0), 1e-6)
        start = t0 + float(np.linalg.norm(np.asarray(ag.position, dtype=float) - np.asarray(t.position))) / v
        dl = getattr(t, "hard_deadline", None)
        if dl is not None and start > float(dl) + 1e-6:
            return math.inf
        c = 0.0 + start
        if dl is not None and start > float(dl):
            c += 200.0 + (start - float(dl))
        cap = float(ag.currentCap2Task[t.typeIdx])
        c -= 5.0 * (max(cap, 0.5) if is_coalition(t) else cap)
        return c

    def plan(self, live, tasks, now, events, known_map=None):
        """[(agent, task)] in live order, or None when the gate holds the plan back."""
        self.n_calls += 1
        if not self.gate(now, events):
            return None
        self.last_plan_step = now
        self.n_replans += 1
        live = [a for a in live if getattr(a, "state", 0) != -1]
        sl = self.slots(tasks) if live and tasks else []
        if not sl:
            return []
        owner = {k: None for k, _ in sl}   # slot key -> (agent id, rpi)
        held = {}                          # agent id -> slot key
        # eligibility and cost do not change within a plan: (cost, slot key) of every eligible, feasible pair, per agent
        pairs = {}
        for ag in live:
            known = None if known_map is None else known_map.get(ag.name, set())
            row, memo = [], {}
            for key, t in sl:
                if t.id not in memo:
                    memo[t.id] = self.cost(ag, t, now) if self.eligible(ag, t, known) else math.inf
                if np.isfinite(memo[t.id]):
                    row.append((memo[t.id], key))
            pairs[ag.id] = row
        for _ in range(len(sl) * len(live)):
            best = None
            for ag in live:
                if ag.id in held:
                    continue
                for c, key in pairs[ag.id]:
                    inc = owner[key]
                    if inc is not None and inc[0] == ag.id:
                        continue
                    if inc is not None and (c < inc[1] - 1e-9 or (abs(c - inc[1]) <= 1e-9 and ag.id >= inc[0])):
                        continue
                    if best is None or (c, ag.id, key) < best:
                        best = (c, ag.id, key)
            if best is None:
                break
            c, aid, key = best
            inc = owner[key]
            if inc is not None and inc[0] != aid:
                held.pop(inc[0], None)
            owner[key] = (aid, c)
            held[aid] = key
        tk = dict(sl)
        return [(a, tk[held[a.id]]) for a in live if a.id in held]


def pi_actions(env, pi, events, use_visibility=True):
    res = pi.plan(env.get_live_agents(), open_tasks(env), env.time_steps, events,
                  env.agent_visibility_map() if use_visibility else None)
    acts = {}
    for ag, t in res or []:  # _apply_assign (wps_eval.py:55-61)
        if env.last_tasks_info and t in env.last_tasks_info and ag.name not in acts:
            acts[ag.name] = env.last_tasks_info.index(t)
    return acts, res


def run_episode(env, seed, mode, interval=20, use_visibility=True, metric_keys=None, on_step=None):
    """The harness loop over `env` (reference env or facade).  mode 'pi' / 'cap_greedy'.  Returns dict(actions=[(t, agent id,
    task id, index)], metrics=[...] (metric_keys order), n_replans).  on_step(env, actions) is called before each step."""
    obs, info = env.reset(seed=seed)
    pi = PI(interval)
    rows, latest = [], None
    done = {a: False for a in env.agents}
    trunc = {a: False for a in env.agents}
    while not all(done.values()) and not all(trunc.values()):
        ev = events_of(info)
        if mode == "pi":
            acts, _ = pi_actions(env, pi, ev, use_visibility)
        else:
            acts = cap_greedy_actions(env, use_visibility)
        for name, i in acts.items():
            rows.append((env.time_steps, env.agent_by_name[name].id, env.last_tasks_info[i].id, i))
        if on_step is not None:
            on_step(env, acts)
        obs, rew, done, trunc, info = env.step(acts)
        if isinstance(info, dict) and "metrics" in info:
            latest = info["metrics"]
    out = {"actions": np.array(rows, dtype=np.int64).reshape(-1, 4), "n_replans": pi.n_replans if mode == "pi" else 0}
    if metric_keys is not None and latest is not None:
        out["metrics"] = np.array([float(latest[k]) for k in metric_keys], dtype=np.float64)
    return out
