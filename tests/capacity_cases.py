"""Scenarios that fill one per-env list of a device tile exactly to its compile-time bound, and scenarios that ask for one entry more.

An env on the device lives in a fixed tile (csrc/muavta_state.h: Tile<A, T, H, R, E, Q>); the reference and the CPU oracle keep unbounded lists.  The
contract (DESIGN.md sections 2 and 5) is "capacity is never exceeded silently": the env that needs more sets ERROR to a MUAVTA_ERR_* code and muavta_metrics
returns MUAVTA_E_CAPACITY.  Each guard is one comparison in front of an indexed LDS store, so the two things to show per list are that a list of exactly L
entries still gives the oracle's result, and that the request for entry L + 1 raises exactly that list's code and writes nothing.

A scenario is a GENERATOR over one oracle env: it yields operations (dicts, see `Ops`) and looks at the oracle between them; a driver applies every
operation to the oracle first and, on the GPU, to the device env of the same batch row (tests/test_capacity_cases_cpu.py drives the oracle alone and pins
the counters; tests/test_gpu_capacity.py drives both).  The operation after which the list holds exactly L entries carries tag "fill", the first request
for entry L + 1 carries tag "overflow".  A "fits" scenario goes on with the Hungarian allocator to the end of the episode; an "overflow" scenario repeats
its request for REPEAT more steps.

  limit     code  bound  routes
  queue      2     Q     `call`: UAV.allocate through muavta_call between two steps; `list`: one list-valued row through muavta_step_lists; `steps`: the rows
                         of two consecutive muavta_step calls; `natural`: an episode of the registry case whose deepest queue is exactly Q (golden seeds)
  events     3     E     _create_escort_for pushes two events, _retire_escort one; the list is only cleared when a step starts (sim/step.inc: the drain),
                         so create / retire calls between two steps reach E and E + 1 on every tile
  pending    4     R     every _create_escort_for registers a pending reveal (threat_delay > 0) that stays for threat_delay steps: creates over several gaps
  slots      1     T     muavta_set_slot_cap on a fixed seed list (golden "slot_seeds"): the smallest cap without a flag lies between two bounds read off the oracle
  escorts    6     A     at the limit only: a fleet of exactly A next to a threat list of exactly H, with an escort for every agent on the 16-agent tile and
                         for as many as one event list has room for (E / 2, see escorts_target) on the other two, whose map entries 16 - 23 and
                         48 - 63 no test ever writes

What cannot be exceeded through the ABI, and is therefore covered at the limit only:
  - escorts: create_escort_for (sim/entities.inc) returns at `if (has_escort(recon)) return;` before it appends, a map entry is only removed together with its
    esc_mask bit, and muavta_call rejects agent ids >= n_agents (abi/sim.inc: "agent id out of range") — so n_escorts <= n_agents <= A and `n >= A` in front
    of the append never fires;
  - fleet and threats: muavta_create picks the tile from max(tile_agents, n_agents) and max(tile_threats, n_threats) and refuses what no tile holds
    (abi/handle.inc: "requested tile exceeds 64 agents x 128 task slots x 48 threats"), so `h >= H` in sim/world.inc never fires either.

Out of scope here: task ids past 32000 (ids are 16-bit on the device; an episode creates a few hundred), the RNG-tape bound MUAVTA_ERR_POSITION (tests/rng_blocks.py:
not run on the device), and making the facade raise on a flag (DESIGN.md open item 8: a behaviour change on the facade's hot path).
"""
import json
import os
from collections import namedtuple

import numpy as np

from muavta_amd.params import params_for_case, params_from_config
from muavta_amd.scenarios import CASE_SPECS, WPS_ENV_FLAGS

Tile = namedtuple("Tile", "A T H R E Q")
TILES = {16: Tile(16, 40, 16, 48, 40, 10), 24: Tile(24, 48, 24, 88, 32, 12), 64: Tile(64, 128, 48, 128, 96, 12)}  # csrc/muavta_state.h (pinned by the CPU test)
CODE = {"slots": 1, "queue": 2, "events": 3, "pending": 4, "escorts": 6}  # MUAVTA_ERR_*
BOUND = {"queue": "Q", "events": "E", "pending": "R", "slots": "T", "escorts": "A"}
E_CAPACITY = -4  # MUAVTA_E_CAPACITY
N_STEPS = 150    # WPS_ENV_FLAGS["max_time_steps"]
REPEAT = 22      # steps an overflow scenario keeps repeating its request
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capacity_cases.json")

# The escort configuration with a fleet of exactly A agents and a threat list of exactly H, per tile (the 24-agent one is WPS_escort24's fleet).
FLEET = {16: {"F1": 5, "F2": 3, "R1": 5, "R2": 3}, 24: {"F1": 9, "F2": 5, "R1": 6, "R2": 4}, 64: {"F1": 20, "F2": 12, "R1": 20, "R2": 12}}
THREATS = {16: [("T1", 7), ("T2", 9)], 24: [("T1", 10), ("T2", 14)], 64: [("T1", 20), ("T2", 28)]}
QUEUE_CASE = "WPS_hard_x2"  # the smallest registry case with Q + 1 = 13 resident tasks after reset (14); its 16 agents fit every tile
FULL_DELAY = 6              # "full": reveals stay 6 steps, not WPS_escort24's 15 (whose natural episodes already need 60 of the 16-agent tile's 48 reveals)
INTERVAL = {"WPS_hard_x2": 20, "full": 12, "slow": 12, "WPS_escort24": 12, "WPS_escort": 12, "WPS_burst64": 20}


def full_spec(tile, **over):
    s = dict(CASE_SPECS["WPS_escort24"])
    s.update(agents=dict(FLEET[tile]), threats_list=list(THREATS[tile]), threat_delay=FULL_DELAY)
    s.update(over)
    return s


def params(case, tile):
    """MuavtaParams of `case` on tile `tile` ("full": the A-agent, H-threat escort configuration of that tile)."""
    tl = TILES[tile]
    if case in ("full", "slow"):
        # "slow": reveals stay WPS_escort24's 15 steps, and nothing but the scenario's own calls registers one: no arrivals, no threats to pop up, and no
        # Rec task for whose recon UAV a step would create an escort (a list that holds exactly R reveals has no room for the episode's own)
        over = {} if case == "full" else {"threat_delay": 15, "arrival_rate": 0.0, "threats_list": [], "tasks": {"Att": 14, "Rec": 0, "Hold": 0}}
        return params_from_config(full_spec(tile, **over), dict(WPS_ENV_FLAGS), tile_agents=tl.A, tile_tasks=tl.T, tile_threats=tl.H)
    return params_for_case(case, tile_agents=tl.A, tile_tasks=tl.T, tile_threats=tl.H)


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------------------------- operations
class Ops:
    """What a scenario yields.  `call`: one muavta_call; `create_all` / `retire_all`: _create_escort_for for every agent / _retire_escort for every map
    entry OF THE SIDE THAT APPLIES IT (after a flag the device's map is no longer the oracle's); `step`: explicit list-valued actions [(agent, index into
    last_tasks_info)], `lists=True` forcing muavta_step_lists; `plan`: the Hungarian allocator's actions.  Every step, of either kind, runs the allocator first
    (the batch has one allocate call per step), so the allocator's own counters stay equal on both sides."""

    @staticmethod
    def reset(seed):
        return {"op": "reset", "seed": int(seed)}

    @staticmethod
    def call(name, iargs, tag=None):
        return {"op": "call", "name": name, "iargs": tuple(int(x) for x in iargs), "tag": tag}

    @staticmethod
    def create_all(rec):
        return {"op": "create_all", "rec": int(rec), "tag": None}

    @staticmethod
    def retire_all():
        return {"op": "retire_all", "tag": None}

    @staticmethod
    def step(actions=(), lists=False, tag=None):
        return {"op": "step", "actions": [(int(a), int(i)) for a, i in actions], "lists": bool(lists), "tag": tag}

    @staticmethod
    def plan(tag=None):
        return {"op": "plan", "tag": tag}


OPS = {"uav_allocate": 0, "create_escort": 1, "sync_escorts": 2, "retire_escort": 3}


def oracle_call(o, name, iargs):
    import orc
    ia = np.zeros(8, dtype=np.int32)
    ia[: len(iargs)] = iargs
    out = np.zeros(72, dtype=np.int32)
    assert o.L.orc_call(o.h, OPS[name], orc._p(ia), orc.C.c_double(-1.0), orc._p(out)) == 0
    return out


def oracle_escorts(o):
    import orc
    out = np.full((64, 2), -1, dtype=np.int32)
    n = o.L.orc_get_escorts(o.h, orc._p(out), 64)
    return out[:n]


def apply_oracle(o, op, interval):
    """One operation on the oracle; for a step: the actions it was stepped with."""
    k = op["op"]
    if k == "reset":
        o.reset(op["seed"])
    elif k == "call":
        oracle_call(o, op["name"], op["iargs"])
    elif k == "create_all":
        for a in range(o.A):
            oracle_call(o, "create_escort", (a, op["rec"]))
    elif k == "retire_all":
        for _, t in oracle_escorts(o):
            oracle_call(o, "retire_escort", (int(t), 0))
    else:
        aa, ai = o.allocate(interval, 1)
        acts = list(zip(aa.tolist(), ai.tolist())) if k == "plan" else op["actions"]
        o.step([a for a, _ in acts], [i for _, i in acts])
        return acts
    return None


def counters(o):
    """Lengths of the bounded lists, on the oracle: deepest queue, events waiting for the next drain, events the last step drained, pending reveals, escort
    map entries, task ids a device slot is held for (not retired, or queued by a live agent), ids handed out so far, open tasks at the last observation."""
    d, ls = o.dims(), o.list_sizes()
    return {"queue": d["max_queue"], "events": ls["n_event_list"], "drained": d["n_events"], "pending": ls["n_pending"], "escorts": ls["n_escorts"],
            "held": ls["n_held"], "ids": d["n_task_ids"] - 1, "open": d["n_open"], "t": d["time_steps"], "done": bool(d["terminated"] or d["truncated"])}


def within(tl, before, after, stepped):
    """Does the tile hold what the oracle held around one operation?  The slot need of a step is bounded by the slots held before it plus the ids it created
    (no slot is given back before the end-of-step GC unless the tile is full); between steps it is the held count itself."""
    need = before["held"] + (after["ids"] - before["ids"]) if stepped else after["held"]
    return (after["queue"] <= tl.Q and after["events"] <= tl.E and after["drained"] <= tl.E and after["pending"] <= tl.R and after["escorts"] <= tl.A and
            need <= tl.T)


# ---------------------------------------------------------------------------------------------------------------- scenario pieces
def _alive(o):
    rows = o.agents()[0]
    return [a for a in range(o.A) if int(rows[a, 2]) != -1]


def _queue_of(o, a):
    q = o.agents()[2][a]
    return [int(t) for t in q if t > 0]


def _tail(o):
    while not counters(o)["done"]:
        yield Ops.plan()


def _queue_requests(o, tl):
    """agent, the ids that fill its queue to Q, and one id more: open (status != 2) tasks of the last observation it does not queue yet"""
    a = _alive(o)[0]
    have = _queue_of(o, a)
    status = o.tasks()[0][:, 0].astype(int)
    cands = [t for t in o.open_ids().tolist() if t not in have and status[t] != 2]
    need = tl.Q - len(have)
    if need < 1 or len(cands) < need + 1:
        raise ValueError(f"agent {a} queues {len(have)}, {len(cands)} more tasks are open: no room for a queue of {tl.Q} + 1")
    return a, cands[:need], cands[need]


def _index(o, t):
    return o.open_ids().tolist().index(t)


def _after_overflow(request):
    """the overflowing request again, before each of REPEAT more steps"""
    for _ in range(REPEAT):
        yield from request()
        yield Ops.step()


def _repeat_step_requests(o, a, extra, lists):
    """REPEAT more steps, each one a request for a task the device's full queue does not hold: `extra` while it is open, then any open task agent `a` does
    not queue on the oracle (whose queue is the device's plus what the device refused)"""
    for _ in range(REPEAT):
        open_ids = o.open_ids().tolist()
        status = o.tasks()[0][:, 0].astype(int)
        have = _queue_of(o, a)
        want = [extra] if extra in open_ids and status[extra] != 2 else [t for t in open_ids if t not in have and status[t] != 2]
        if not want:
            raise ValueError("no open task left to request")
        yield Ops.step([(a, open_ids.index(want[0]))], lists=lists)


def queue_call(o, tl, seed, overflow):
    yield Ops.reset(seed)
    yield Ops.plan()
    yield Ops.plan()
    a, fill, extra = _queue_requests(o, tl)
    t = counters(o)["t"]
    for k, task in enumerate(fill):
        yield Ops.call("uav_allocate", (a, task, t), tag="fill" if k == len(fill) - 1 else None)
    if not overflow:
        yield from _tail(o)
        return
    yield Ops.call("uav_allocate", (a, extra, t), tag="overflow")
    yield Ops.step()

    def again():
        yield Ops.call("uav_allocate", (a, extra, counters(o)["t"]))
    yield from _after_overflow(again)


def queue_list(o, tl, seed, overflow):
    yield Ops.reset(seed)
    yield Ops.plan()
    a, fill, extra = _queue_requests(o, tl)
    yield Ops.step([(a, _index(o, t)) for t in fill], lists=True, tag="fill")
    if not overflow:
        yield from _tail(o)
        return
    yield Ops.step([(a, _index(o, extra))], lists=True, tag="overflow")
    yield from _repeat_step_requests(o, a, extra, True)


def queue_steps(o, tl, seed, overflow):
    yield Ops.reset(seed)
    a, fill, extra = _queue_requests(o, tl)
    yield Ops.step([(a, _index(o, t)) for t in fill[:-3]])
    yield Ops.step([(a, _index(o, t)) for t in fill[-3:]], tag="fill")
    if not overflow:
        yield from _tail(o)
        return
    yield Ops.step([(a, _index(o, extra))], tag="overflow")
    yield from _repeat_step_requests(o, a, extra, False)


def natural(o, tl, seed, overflow=False):
    yield Ops.reset(seed)
    yield from _tail(o)


def _fill_events(o, tl, upto):
    """create / retire calls until the event list holds `upto` entries (a create adds two, a retire one); the last one tagged "fill" """
    rec = o.open_ids().tolist()[0]
    while True:
        n = counters(o)["events"]
        if n >= upto:
            if n > upto:
                raise ValueError(f"the event list already holds {n} > {upto}")
            return
        esc = oracle_escorts(o)
        free = [a for a in _alive(o) if a not in set(esc[:, 0].tolist())]
        last = lambda add: "fill" if n + add == upto else None
        if upto - n >= 2 and free:
            yield Ops.call("create_escort", (free[0], rec), tag=last(2))
        elif len(esc):
            yield Ops.call("retire_escort", (int(esc[0, 1]), 0), tag=last(1))
        else:
            raise ValueError("no escort to retire and no room for a create")


def _hammer(o):
    """more events and pending reveals than any tile holds, before each of REPEAT more steps"""
    for _ in range(REPEAT):
        rec = o.open_ids().tolist()[0]
        yield Ops.create_all(rec)
        yield Ops.retire_all()
        yield Ops.create_all(rec)
        yield Ops.step()


def events(o, tl, seed, overflow):
    yield Ops.reset(seed)
    yield Ops.plan()
    yield from _fill_events(o, tl, tl.E)
    if not overflow:
        yield from _tail(o)
        return
    yield Ops.call("retire_escort", (int(oracle_escorts(o)[0, 1]), 0), tag="overflow")
    yield Ops.step()
    yield from _hammer(o)


def pending(o, tl, seed, overflow, max_gaps=14):
    """Creates in every gap, as many as the event list and the slots leave room for (every step retires the escorts again, one event each); the gap in
    which the rest fits fills the list to exactly R."""
    yield Ops.reset(seed)
    for gap in range(max_gaps):
        rec = o.open_ids().tolist()[0]
        while True:
            c = counters(o)
            esc = oracle_escorts(o)
            free = [a for a in _alive(o) if a not in set(esc[:, 0].tolist())]
            ev_room, slot_room, missing = tl.E - c["events"], tl.T - c["held"] - 4, tl.R - c["pending"]
            # can the rest be done in this gap?  a create on a free agent costs 2 events, on a busy one 3 (retire first)
            cost = 2 * min(missing, len(free)) + 3 * max(missing - len(free), 0)
            finishing = cost <= ev_room and missing <= slot_room + 4 and (missing <= len(free) or len(esc) > 0)
            if missing == 0:
                break
            if not finishing and (ev_room < 2 or slot_room < 1 or not free):
                break
            if free:
                yield Ops.call("create_escort", (free[0], rec), tag="fill" if missing == 1 else None)
            else:
                yield Ops.call("retire_escort", (int(esc[0, 1]), 0))
        if counters(o)["pending"] == tl.R:
            break
        yield Ops.plan()
    else:
        raise ValueError(f"pending reveals {counters(o)['pending']} after {max_gaps} gaps, wanted {tl.R}")
    if not overflow:
        yield from _tail(o)
        return
    esc = oracle_escorts(o)
    free = [a for a in _alive(o) if a not in set(esc[:, 0].tolist())]
    if not free:
        yield Ops.call("retire_escort", (int(esc[0, 1]), 0))
        free = [int(esc[0, 0])]
    yield Ops.call("create_escort", (free[0], o.open_ids().tolist()[0]), tag="overflow")
    yield Ops.step()
    yield from _hammer(o)


def queue_then_events(o, tl, seed, overflow=True):
    """fail() keeps the FIRST code: the queue overflows, then the event list does"""
    yield Ops.reset(seed)
    yield Ops.plan()
    a, fill, extra = _queue_requests(o, tl)
    t = counters(o)["t"]
    for k, task in enumerate(fill):
        yield Ops.call("uav_allocate", (a, task, t), tag="fill" if k == len(fill) - 1 else None)
    yield Ops.call("uav_allocate", (a, extra, t), tag="overflow")
    yield Ops.step()
    yield from _hammer(o)


def escorts_target(tl):
    """Escort map entries the ABI can put side by side: every create pushes two events into the list of one step, and the Reset_Allocation among them
    empties every queue when the next step drains it, which retires the escorts (their UAVs are idle then) — A on the 16-agent tile (2 A <= E), E / 2 of
    the A on the other two."""
    return min(tl.A, tl.E // 2)


def escorts_full(o, tl, seed, overflow=False):
    """An escort for every agent the event list has room for, in the fleet of exactly A next to the threat list of exactly H: every agent is sent to an
    open task first and gets the escort for that task."""
    yield Ops.reset(seed)
    status = o.tasks()[0][:, 0].astype(int)
    open_ids = [t for t in o.open_ids().tolist() if status[t] != 2]
    want = escorts_target(tl)
    for k, a in enumerate(_alive(o)[:want]):
        task = open_ids[a % len(open_ids)]
        yield Ops.call("uav_allocate", (a, task, 0))
        yield Ops.call("create_escort", (a, task), tag="fill" if k == want - 1 else None)
    yield from _tail(o)


BUILDERS = {"queue_call": queue_call, "queue_list": queue_list, "queue_steps": queue_steps, "queue_natural": natural, "events": events, "pending": pending,
            "queue_then_events": queue_then_events, "escorts_full": escorts_full, "benign": natural}
LIMIT_OF = {"queue_call": "queue", "queue_list": "queue", "queue_steps": "queue", "queue_natural": "queue", "events": "events", "pending": "pending",
            "queue_then_events": "queue", "escorts_full": "escorts", "benign": None}
CASE_OF = {"queue_call": QUEUE_CASE, "queue_list": QUEUE_CASE, "queue_steps": QUEUE_CASE, "events": "full", "pending": "slow", "queue_then_events": "full",
           "escorts_full": "full"}


class Scenario:
    def __init__(self, builder, tile, kind, seed, case=None):
        self.builder, self.tile, self.kind, self.seed = builder, int(tile), kind, int(seed)
        self.case = case or CASE_OF[builder]
        self.limit = LIMIT_OF[builder]
        self.tl = TILES[self.tile]
        self.interval = INTERVAL[self.case]
        self.name = f"{builder}-{kind}-{self.tile}-{self.case}-s{seed}"

    bound = property(lambda self: escorts_target(self.tl) if self.limit == "escorts" else getattr(self.tl, BOUND[self.limit]))
    code = property(lambda self: CODE[self.limit])

    def params(self):
        return params(self.case, self.tile)

    def ops(self, o):
        return BUILDERS[self.builder](o, self.tl, self.seed, self.kind == "overflow")

    def __repr__(self):
        return self.name


def run_on_oracle(sc, o=None, stop_at=None):
    """The scenario on the oracle alone: [(op, counters before, counters after)].  `stop_at`: stop after the operation with that tag."""
    import orc
    o = o or orc.OracleEnv(sc.params())
    trace = []
    before = None
    for op in sc.ops(o):
        apply_oracle(o, op, sc.interval)
        after = counters(o)
        trace.append((op, before, after))
        before = after
        if stop_at and op.get("tag") == stop_at:
            break
    return trace, o


def check_trace(sc, trace):
    """What makes the GPU test of the scenario mean something, as (ok, why): a "fits" scenario reaches exactly the bound at its "fill" and never more, and the
    tile holds everything else for the whole episode; an "overflow" scenario stands at the bound before its "overflow" request and one past it after, and
    the tile held everything up to there."""
    tl, L = sc.tl, None
    if sc.limit:
        L = sc.bound
    ops = [t[0] for t in trace]
    tags = [op.get("tag") for op in ops]
    fine = [i == 0 or within(tl, b, a, op["op"] in ("step", "plan")) for i, (op, b, a) in enumerate(trace)]
    if sc.kind == "benign":
        return (all(fine), "within the tile") if all(fine) else (False, f"outgrows the tile at operation {fine.index(False)}")
    key = sc.limit
    if sc.builder == "queue_natural":
        peak = max(a["queue"] for _, _, a in trace)
        if sc.kind == "fits":
            return (peak == L and all(fine)), f"peak queue {peak}, within the tile otherwise: {all(fine)}"
        return peak > L, f"peak queue {peak}"
    if "fill" not in tags:
        return False, "no fill operation"
    at = tags.index("fill")
    if trace[at][2][key] != L:
        return False, f"{key} is {trace[at][2][key]} after the fill, wanted {L}"
    if sc.kind == "fits":
        peak = max(max(a[key], a["drained"]) if key == "events" else a[key] for _, _, a in trace)
        if peak != L:
            return False, f"{key} peaks at {peak}, wanted {L}"
        if not all(fine):
            return False, f"outgrows the tile at operation {fine.index(False)}: {trace[fine.index(False)][2]}"
        if not trace[-1][2]["done"]:
            return False, "the episode did not end"
        return True, f"{key} == {L} at operation {at}"
    if "overflow" not in tags:
        return False, "no overflow operation"
    ov = tags.index("overflow")
    if not all(fine[:ov]):
        return False, f"outgrows the tile before the overflow, at operation {fine.index(False)}"
    b, a = trace[ov][1], trace[ov][2]
    if b[key] != L or a[key] != L + 1:
        return False, f"{key} goes {b[key]} -> {a[key]} at the overflow, wanted {L} -> {L + 1}"
    if any(a[k] > getattr(tl, BOUND[k]) for k in ("queue", "events", "pending") if k != key) or a["held"] > tl.T:
        return False, "another list overflows with the same request"
    # the request is repeated before (a call) or in (a row of actions) at least 20 more steps
    n_after, asked = 0, False
    for op in ops[ov + 1:]:
        if op["op"] in ("call", "create_all"):
            asked = True
        elif op["op"] == "step":
            n_after += asked or bool(op["actions"])
            asked = False
    if n_after < 20:
        return False, f"only {n_after} steps with the request repeated after the overflow"
    if sc.builder == "queue_then_events" and not any(a["events"] > tl.E for _, _, a in trace[ov:]):
        return False, "the event list never overflows after the queue did"
    return True, f"{key} {L} -> {L + 1} at operation {ov}"


# ---------------------------------------------------------------------------------------------------------------- the scenario set
def scenarios():
    """Every constructed scenario and the natural episodes, seeds from tests/golden/capacity_cases.json (tools/find_capacity_cases.py)."""
    out = []
    for row in golden()["scenarios"]:
        out.append(Scenario(row["builder"], row["tile"], row["kind"], row["seed"], row.get("case")))
    return out


MODES = {"hungarian": 0, "urgency_pair": 1, "urgency_coalition": 2, "hungarian_gated": 3}  # allocators the oracle restates


def natural_peaks(case, tile, seed, mode="hungarian", o=None):
    """deepest queue, longest pending-reveal and event lists and largest slot need after any step of the episode the allocator `mode` plays from `seed`"""
    import orc
    o = o or orc.OracleEnv(params(case, tile))
    o.reset(seed)
    q = p = ev = need = 0
    c = counters(o)
    for _ in range(N_STEPS):
        aa, ai = o.allocate_mode(INTERVAL[case], 1, MODES[mode])
        done = o.step(aa, ai)
        n = counters(o)
        q, p, ev = max(q, n["queue"]), max(p, n["pending"]), max(ev, n["events"], n["drained"])
        need = max(need, c["held"] + n["ids"] - c["ids"], n["held"])
        c = n
        if done:
            break
    return {"queue": q, "pending": p, "events": ev, "slots": need}


# ---------------------------------------------------------------------------------------------------------------- task slots
def slot_bounds(case, tile, seed, interval):
    """Bounds on the smallest slot cap an episode runs under without a flag, read off the oracle: at least the most open tasks of any observation, at most
    the most slots the device's holding rule can ask for (held before a step + ids the step creates; held count between steps)."""
    import orc
    o = orc.OracleEnv(params(case, tile))
    o.reset(seed)
    c = counters(o)
    lo, hi = c["open"], c["held"]
    while not c["done"]:
        aa, ai = o.allocate(interval, 1)
        o.step(aa, ai)
        n = counters(o)
        lo = max(lo, n["open"])
        hi = max(hi, c["held"] + n["ids"] - c["ids"], n["held"])
        c = n
    return lo, hi


# ---------------------------------------------------------------------------------------------------------------- the raw counts of a flagged env
# muavta_get clamps what it returns to the tile (k < n_events ...), so "the count stayed within the tile" has to be read from the state record itself
# (muavta_get_state): offsets from a host program that includes csrc/muavta_state.h, as tests/test_mlp_pair_cpu.py does for the ABI structs.
_LAYOUT_FIELDS = ["a_qslot", "a_qlen", "pend_slot", "n_events", "n_dev", "n_pending", "n_escorts", "n_order", "n_open", "error"]
_layout = None


def state_layout(workdir=None):
    global _layout
    if _layout is None:
        import subprocess
        import tempfile
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        workdir = workdir or tempfile.mkdtemp(prefix="muavta_layout_")
        fmt = " ".join(f"{f} %zu" for f in _LAYOUT_FIELDS)
        args = ", ".join(f"offsetof(S, {f})" for f in _LAYOUT_FIELDS)
        src = ['#include <cstdio>', '#include <cstddef>', '#include "muavta_state.h"', 'template <class TL> void show(int n) {', '  typedef EnvState<TL> S;',
               f'  printf("%d sizeof %zu A %d T %d H %d R %d E %d Q %d {fmt}\\n", n, sizeof(S), TL::A, TL::T, TL::H, TL::R, TL::E, TL::Q, {args});', '}',
               'int main() { show<Tile16>(16); show<Tile24>(24); show<Tile64>(64); return 0; }']
        path = os.path.join(workdir, "layout.cpp")
        with open(path, "w") as f:
            f.write("\n".join(src) + "\n")
        exe = os.path.join(workdir, "layout")
        subprocess.check_call(["g++", "-std=c++17", "-w", "-I", os.path.join(root, "multi-uav-ta-gym-env_amd", "csrc"), "-o", exe, path])
        _layout = {}
        for line in subprocess.check_output([exe], text=True).splitlines():
            w = line.split()
            _layout[int(w[0])] = {k: int(v) for k, v in zip(w[1::2], w[2::2])}
    return _layout


def raw_counts(state, tile, i, n_agents):
    """The list lengths and slot indices env i's record holds, as stored (buffer of muavta_get_state: the n_envs EnvState records come first)."""
    lay, tl = state_layout()[tile], TILES[tile]
    rec = np.asarray(state, dtype=np.uint8)[i * lay["sizeof"]: (i + 1) * lay["sizeof"]]
    i32 = lambda f: int(rec[lay[f]: lay[f] + 4].view(np.int32)[0])
    qlen = rec[lay["a_qlen"]: lay["a_qlen"] + tl.A].view(np.int8)[:n_agents].astype(int)
    qslot = rec[lay["a_qslot"]: lay["a_qslot"] + tl.A * tl.Q].view(np.int8).reshape(tl.A, tl.Q)[:n_agents].astype(int)
    out = {f: i32(f) for f in ("n_events", "n_dev", "n_pending", "n_escorts", "n_order", "n_open", "error")}
    out["a_qlen"] = qlen
    out["queue_slots"] = [int(qslot[a, k]) for a in range(n_agents) for k in range(max(0, min(int(qlen[a]), tl.Q)))]
    out["pend_slots"] = rec[lay["pend_slot"]: lay["pend_slot"] + max(0, min(out["n_pending"], tl.R))].astype(int).tolist()
    return out
