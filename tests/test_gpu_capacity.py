"""The device at every per-env capacity of its tiles: a list filled exactly to its compile-time bound still gives the oracle's result, stepwise and in the
fused rollout; the first request past the bound sets ERROR to that list's code, keeps it, leaves every count and index of the flagged env inside the tile
for as long as it is driven on, disturbs no neighbour, and is gone after a reset.  Scenarios: tests/capacity_cases.py (pinned to the oracle on the CPU by
tests/test_capacity_cases_cpu.py); no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import capacity_cases as cc
import orc
from test_gpu_parity import Snapshot, compare

pytestmark = pytest.mark.gpu

TILES = list(cc.TILES)
CASES = [cc.QUEUE_CASE, "full", "slow"]


def _handle(p, n):
    from muavta_amd.batched import BatchedMultiUAVEnv
    return BatchedMultiUAVEnv(p, n)


def _metrics_rc(env):
    m = np.empty((env.n_envs, 30), dtype=np.float64)
    return env.L.muavta_metrics(env.h, m.ctypes.data_as(C.c_void_p))


class Row:
    def __init__(self, sc):
        trace, _ = cc.run_on_oracle(sc)
        ok, why = cc.check_trace(sc, trace)
        assert ok, f"{sc.name}: {why}"  # (also pinned on the CPU; here it costs a few milliseconds and keeps a vacuous run from passing)
        self.sc = sc
        self.o = orc.OracleEnv(sc.params())
        self.gen = sc.ops(self.o)
        self.applied, self.step_op = [], None
        self.filled = sc.kind == "benign" or sc.builder == "queue_natural"
        self.flagged = self.exhausted = False
        self.fused_want = None

    def next_op(self):
        try:
            return next(self.gen)
        except StopIteration:
            self.exhausted = True
            return None


def _device_between(env, i, op):
    k = op["op"]
    if k == "call":
        env.call(op["name"], op["iargs"], env_index=i)
    elif k == "create_all":
        for a in range(env.n_agents):
            env.call("create_escort", (a, op["rec"]), env_index=i)
    elif k == "retire_all":
        for a, t in env.get("ESCORTS")[i]:
            if a >= 0:
                env.call("retire_escort", (int(t), 0), env_index=i)
    else:
        raise AssertionError(k)


def _within_the_tile(env, tile, snap, state, i, row, tag):
    """every count and index env i's record holds, as stored, stays inside the tile"""
    tl = cc.TILES[tile]
    raw = cc.raw_counts(state, tile, i, env.n_agents)
    assert raw["error"] == row.sc.code, f"{tag}: ERROR {raw['error']}, the first code was {row.sc.code}"
    assert snap.ERROR[i] == row.sc.code
    assert raw["a_qlen"].min() >= 0 and raw["a_qlen"].max() <= tl.Q, f"{tag}: a_qlen {raw['a_qlen']}"
    assert 0 <= raw["n_events"] <= tl.E and 0 <= raw["n_dev"] <= tl.E, f"{tag}: n_events {raw['n_events']} n_dev {raw['n_dev']}"
    assert 0 <= raw["n_pending"] <= tl.R, f"{tag}: n_pending {raw['n_pending']}"
    assert 0 <= raw["n_escorts"] <= tl.A, f"{tag}: n_escorts {raw['n_escorts']}"
    assert 0 <= raw["n_order"] <= tl.T and 0 <= raw["n_open"] <= tl.T, f"{tag}: n_order (live slots) {raw['n_order']}, n_open {raw['n_open']}"
    assert all(0 <= s < tl.T for s in raw["queue_slots"]), f"{tag}: queue slot indices {raw['queue_slots']}"
    assert all(0 <= s < tl.T for s in raw["pend_slots"]), f"{tag}: pending slot indices {raw['pend_slots']}"


def drive(env, tile, rows, want_fused):
    """The rows' scenarios in lockstep on one handle: calls between steps go to the row's env, a step is one batch step.  Runs until every fits row has
    finished its episode, or every overflow row its repeats.  Returns the fused-rollout result taken from the state in which every row had its list filled
    (fits) or its flag raised (overflow): (t, metrics, ERROR) of a second handle that ran rollout(None, remaining steps) from a copy of that state."""
    interval = rows[0].sc.interval
    p = rows[0].sc.params()
    driving = [r for r in rows if r.sc.kind != "benign"] or rows
    seeds = []
    for r in rows:
        op = r.next_op()
        assert op["op"] == "reset"
        cc.apply_oracle(r.o, op, interval)
        r.applied.append(op)
        seeds.append(op["seed"])
    env.reset(np.array(seeds, dtype=np.uint64))
    snap = Snapshot(env)
    for i, r in enumerate(rows):
        compare(snap, i, r.o, f"{r.sc.name} after reset")
    t, fused = 0, None
    while True:
        for i, r in enumerate(rows):  # ---- between two steps
            r.step_op = None
            while not r.exhausted:
                op = r.next_op()
                if op is None:
                    break
                if op["op"] in ("step", "plan"):
                    r.step_op = op
                    break
                cc.apply_oracle(r.o, op, interval)
                _device_between(env, i, op)
                r.applied.append(op)
                if op["tag"] == "fill":
                    r.filled = True
                    compare(Snapshot(env), i, r.o, f"{r.sc.name} t={t} after the filling call", check_obs=False)
                elif op["tag"] == "overflow":
                    r.flagged = True
                    err = env.get("ERROR")
                    assert err[i] == r.sc.code, f"{r.sc.name}: ERROR {err[i]} after the first request past the bound, wanted {r.sc.code}"
                    assert all(err[j] == 0 for j, x in enumerate(rows) if not x.flagged), f"{r.sc.name}: neighbours flagged {err}"
        if all(r.exhausted for r in driving):
            break
        if want_fused and fused is None and all(r.filled for r in rows) and all(r.flagged for r in driving if r.sc.kind == "overflow"):
            # ---- the fused kernels from this state, on a second handle
            h2 = _handle(p, len(rows))
            try:
                h2.set_state(env.get_state())
                h2.set_rng(env.get_rng())
                h2.rollout(None, cc.N_STEPS - t, interval, True, True)
                fused = (t, h2.rollout_metrics(), h2.get("ERROR").copy(), _metrics_rc(h2))
            finally:
                h2.close()
            for r in rows:
                if not r.flagged:
                    o2 = orc.OracleEnv(p)
                    for op in r.applied:
                        cc.apply_oracle(o2, op, interval)
                    o2.rollout(r.sc.seed, cc.N_STEPS - t, interval, 1, 0)
                    r.fused_want = o2.metrics()
        # ---- one batch step: the allocator runs for every env (its counters are state too), explicit rows replace its actions
        aa_d, ai_d = env.allocate(interval, True)
        per_env, lists, ops = [], False, []
        for i, r in enumerate(rows):
            op = r.step_op or cc.Ops.step()
            acts = cc.apply_oracle(r.o, op, interval)
            if op["op"] == "plan":
                k = len(acts)
                assert [int(x) for x in aa_d[i][:k]] == [a for a, _ in acts] and np.all(aa_d[i][k:] == -1), f"{r.sc.name} t={t}: planned agents"
                assert [int(x) for x in ai_d[i][:k]] == [j for _, j in acts], f"{r.sc.name} t={t}: planned indices"
            per_env.append(acts)
            lists |= op["lists"] if op["op"] == "step" else False
            r.applied.append(op)
            ops.append(op)
        aa, ai = env.pack_actions(per_env)
        if lists and aa.shape[1] == env.A_tile:  # (a row no longer than action_cap goes through muavta_step_lists when the arrays are wider)
            aa = np.concatenate([aa, np.full((len(rows), 1), -1, np.int32)], axis=1)
            ai = np.concatenate([ai, np.zeros((len(rows), 1), np.int32)], axis=1)
        env.step(aa, ai)
        t += 1
        snap = Snapshot(env)
        state = env.get_state() if any(r.flagged or op["tag"] == "overflow" for r, op in zip(rows, ops)) else None
        for i, (r, op) in enumerate(zip(rows, ops)):
            if op["tag"] == "fill":
                r.filled = True
            elif op["tag"] == "overflow":
                r.flagged = True
            if r.flagged:
                _within_the_tile(env, tile, snap, state, i, r, f"{r.sc.name} t={t}")
            else:
                compare(snap, i, r.o, f"{r.sc.name} t={t}")
    return fused


def _rows(tile, case, kind):
    scs = [s for s in cc.scenarios() if s.tile == tile and s.case == case and s.kind == kind]
    benign = [cc.Scenario("benign", tile, "benign", s, case) for s in cc.golden()["benign"][str(tile)][case]]
    return scs, benign


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tile", TILES)
def test_a_list_filled_exactly_to_its_bound_gives_the_oracles_result(tile, case):
    """ERROR == 0 and every field of every env equal to the oracle after the filling operation and after every step to the end of the episode; the fused
    rollout from the filled state ends with the metrics of the stepwise path and of the oracle."""
    scs, benign = _rows(tile, case, "fits")
    assert scs
    rows = [Row(s) for s in scs + benign[:1]]
    assert len(rows) <= 8
    env = _handle(rows[0].sc.params(), len(rows))
    try:
        assert (env.A_tile, env.T, env.Q, env.E) == (cc.TILES[tile].A, cc.TILES[tile].T, cc.TILES[tile].Q, cc.TILES[tile].E)
        fused = drive(env, tile, rows, True)
        assert fused is not None and fused[0] < cc.N_STEPS - 100, "no fused rollout from the filled state"
        assert not env.get("ERROR").any() and not fused[2].any() and fused[3] == 0
        m = env.metrics()
        for i, r in enumerate(rows):
            want = r.o.metrics()
            assert np.array_equal(m[i], want), f"{r.sc.name}: stepwise metrics"
            assert np.array_equal(fused[1][i], want) and np.array_equal(r.fused_want, want), f"{r.sc.name}: fused metrics from t={fused[0]}"
    finally:
        env.close()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tile", TILES)
def test_the_first_request_past_a_bound_flags_that_env_alone(tile, case):
    """Overflowing envs at the middle indices, benign envs of other seeds on both sides.  The code is the list's, it stays (queue_then_events: the event list
    overflows later), muavta_metrics reports MUAVTA_E_CAPACITY, the flagged env's counts and indices stay inside the tile while it is driven on with the
    request repeated every step, the neighbours stay equal to their oracles stepwise and fused, and a reset leaves nothing behind."""
    scs, benign = _rows(tile, case, "overflow")
    assert scs and len(benign) >= 2 * len(scs) + 2
    order = []
    for k, s in enumerate(scs):
        order += [benign[k], s]
    order.append(benign[len(scs)])
    rows = [Row(s) for s in order]
    assert len(rows) <= 8 and rows[0].sc.kind == rows[-1].sc.kind == "benign"
    env = _handle(rows[0].sc.params(), len(rows))
    try:
        fused = drive(env, tile, rows, True)
        assert fused is not None
        err = env.get("ERROR")
        for i, r in enumerate(rows):
            if r.sc.kind == "overflow":
                assert r.flagged and err[i] == r.sc.code and fused[2][i] == r.sc.code, f"{r.sc.name}: ERROR {err[i]}, fused {fused[2][i]}, wanted {r.sc.code}"
            else:
                assert err[i] == 0 and fused[2][i] == 0
                assert np.array_equal(fused[1][i], r.fused_want), f"{r.sc.name}: fused metrics next to a flagged env"
        assert _metrics_rc(env) == cc.E_CAPACITY and fused[3] == cc.E_CAPACITY
        # the same handle after a reset of the whole batch: the flagged indices run a whole benign episode like any other
        again = [Row(s) for s in benign[len(scs) + 1:][:len(rows)]]
        again += [Row(s) for s in benign[:len(rows) - len(again)]]
        drive(env, tile, again, False)
        assert not env.get("ERROR").any() and _metrics_rc(env) == 0
        m = env.metrics()
        for i, r in enumerate(again):
            assert np.array_equal(m[i], r.o.metrics()), f"{r.sc.name} after the flagged batch: metrics"
    finally:
        env.close()


@pytest.mark.parametrize("tile", TILES)
def test_slot_cap_flags_between_the_oracles_two_bounds(tile):
    """muavta_set_slot_cap(c), one handle per cap from the tile's T downwards, three seeds: (a) above the smallest cap c* that raises no flag the episode is
    the oracle's; (b) c* - 1 flags code 1; (c) c* >= the most open tasks of any observation; (d) c* <= the most slots the holding rule can ask for (not retired,
    or queued by a live agent, plus what the step creates).  Then the first seed stepwise under exactly c*: several steps with all c* slots in use."""
    tl = cc.TILES[tile]
    row = cc.golden()["slot_seeds"][str(tile)]
    case, seeds, bounds = row["case"], row["seeds"], row["bounds"]
    interval = cc.INTERVAL[case]
    p = cc.params(case, tile)
    oracles = [orc.OracleEnv(p) for _ in seeds]
    for o, s in zip(oracles, seeds):
        o.rollout(s, cc.N_STEPS, interval, 1, 1)
    cstar = [None] * len(seeds)
    for c in range(tl.T, 0, -1):
        h = _handle(p, len(seeds))
        try:
            if c < tl.T:
                h.set_slot_cap(c)
            h.rollout(np.array(seeds, dtype=np.uint64), cc.N_STEPS, interval, True, True)
            err, m, snap = h.get("ERROR").copy(), h.rollout_metrics(), Snapshot(h)
            rc = _metrics_rc(h)
        finally:
            h.close()
        assert rc == (cc.E_CAPACITY if err.any() else 0)
        for i, o in enumerate(oracles):
            if err[i] == 0:
                assert cstar[i] is None, f"seed {seeds[i]}: cap {c} raises no flag, cap {cstar[i] - 1} did"
                assert np.array_equal(m[i], o.metrics()), f"seed {seeds[i]} cap {c}: metrics"
                compare(snap, i, o, f"seed {seeds[i]} cap {c}")
            else:
                assert err[i] == cc.CODE["slots"], f"seed {seeds[i]} cap {c}: ERROR {err[i]}"
                if cstar[i] is None:
                    cstar[i] = c + 1
        if all(x is not None for x in cstar):
            break
    print(f"tile {tile}: smallest caps {cstar}, oracle bounds {bounds}")
    for i, (lo, hi) in enumerate(bounds):
        assert cstar[i] <= tl.T, f"seed {seeds[i]}: flagged with all {tl.T} slots"
        assert lo <= cstar[i] <= hi, f"seed {seeds[i]}: smallest cap {cstar[i]}, oracle bounds [{lo}, {hi}]"
    # the full tile, step by step
    sc = cc.Scenario("benign", tile, "benign", seeds[0], case)
    r = Row(sc)
    env = _handle(p, 1)
    try:
        env.set_slot_cap(cstar[0])
        op = r.next_op()
        cc.apply_oracle(r.o, op, interval)
        env.reset(np.array([seeds[0]], dtype=np.uint64))
        full = 0
        for t in range(cc.N_STEPS):
            aa, ai = env.allocate(interval, True)
            cc.apply_oracle(r.o, cc.Ops.plan(), interval)
            env.step(aa, ai)
            snap = Snapshot(env)
            compare(snap, 0, r.o, f"seed {seeds[0]} under cap {cstar[0]} t={t + 1}")
            live = int((snap.TASK_ID[0] >= 0).sum())
            assert live <= cstar[0]
            full += live == cstar[0]
        assert full >= 3, f"only {full} steps with all {cstar[0]} slots in use"
        assert np.array_equal(env.metrics()[0], r.o.metrics())
    finally:
        env.close()


NATURAL_PENDING = cc.golden()["natural_pending"]


@pytest.mark.parametrize("route", NATURAL_PENDING, ids=[f"{r['tile']}-{r['case']}-{r['mode']}" for r in NATURAL_PENDING])
def test_natural_pending_peaks_and_escalation_to_the_next_tile(route):
    """Registry episodes, fused.  WPS_escort24 on the 24-agent tile: under the gated Hungarian the pending-reveal list of the chosen seeds peaks at exactly
    R = 88 and nothing is flagged; under Urgency-Pair two seeds pass R.  WPS_escort on the 16-agent tile under Urgency-Pair: the chosen seeds pass R = 48.
    A seed that passes R is flagged with code 4 and, with escalate=True, gets the oracle's metrics row from the next tile (24 x 48, 64 x 128); every other
    seed of the batch keeps ERROR == 0 and its own row."""
    case, tile, mode = route["case"], route["tile"], route["mode"]
    interval = cc.INTERVAL[case]
    p = cc.params(case, tile)
    over = route["overflow"][:2]
    seeds = route["fits"][:2] + over[:1] + route["below"][:2] + over[1:] + route["fits"][2:3]
    assert len(seeds) >= 3
    env = _handle(p, len(seeds))
    try:
        assert env.A_tile == tile
        env.set_allocator(mode)
        env.rollout(np.array(seeds, dtype=np.uint64), cc.N_STEPS, interval, True, True, escalate=True)
        err = env.get("ERROR")
        for i, s in enumerate(seeds):
            assert err[i] == (cc.CODE["pending"] if s in over else 0), f"{mode} seed {s}: ERROR {err[i]}"
        assert sorted(env.escalated) == [i for i, s in enumerate(seeds) if s in over]
        assert all(h.A_tile == route["next_tile"] and int(h.get("ERROR")[k]) == 0 for h, k in env.escalated.values())
        want = orc.parallel_metrics(p, seeds, interval, 1, cc.MODES[mode], procs=1)
        got = env.rollout_metrics()
        assert np.array_equal(got, want), f"{mode}: rows differing {np.nonzero(~np.all(got == want, axis=1))[0]}"
    finally:
        env.close()


def test_natural_pending_routes_cover_both_escalation_steps():
    assert {r["tile"] for r in NATURAL_PENDING if r["overflow"]} == {16, 24} and any(r["fits"] for r in NATURAL_PENDING)


def test_the_64_agent_tile_reports_the_flag_under_escalation():
    """No tile follows 64 x 128: rollout(escalate=True) of a batch with an overflowing env raises instead of returning a row, the flag stays readable and
    muavta_metrics returns MUAVTA_E_CAPACITY.  No registry episode outgrows this tile, so the overflow is the slot cap's: one slot fewer than the smallest
    cap each seed runs under (the upper bound of the slot test: c* <= hi, so a cap of lo - 1 < c* flags)."""
    from muavta_amd.native import MuavtaError
    tile = 64
    row = cc.golden()["slot_seeds"][str(tile)]
    case, seeds = row["case"], row["seeds"]
    cap = min(lo for lo, _ in row["bounds"]) - 1  # below every seed's lower bound: each env needs more
    env = _handle(cc.params(case, tile), len(seeds))
    try:
        assert env.A_tile == 64 and env.T == 128
        env.set_slot_cap(cap)
        with pytest.raises(MuavtaError, match="no tile left to escalate to"):
            env.rollout(np.array(seeds, dtype=np.uint64), cc.N_STEPS, cc.INTERVAL[case], True, True, escalate=True)
        assert list(env.get("ERROR")) == [cc.CODE["slots"]] * len(seeds) and env.escalated == {}
        assert _metrics_rc(env) == cc.E_CAPACITY
        # without the cap the same handle runs the same seeds clean
        env.set_slot_cap(0)
        env.rollout(np.array(seeds, dtype=np.uint64), cc.N_STEPS, cc.INTERVAL[case], True, True, escalate=True)
        assert not env.get("ERROR").any() and env.escalated == {}
        assert np.array_equal(env.rollout_metrics(), orc.parallel_metrics(cc.params(case, tile), seeds, cc.INTERVAL[case], procs=1))
    finally:
        env.close()


def test_random_lists_flag_the_queue_exactly_when_the_oracles_queue_passes_Q():
    """Random list-valued rows with many distinct tasks per agent (test_list_valued_actions_longer_than_the_tile keeps its lists short): after every step
    ERROR is 2 for exactly the envs whose deepest oracle queue has passed Q, and 0 with every field equal for the others."""
    from muavta_amd.params import params_from_config
    from muavta_amd.scenarios import CASE_SPECS, WPS_ENV_FLAGS
    tile, case, n = 16, cc.QUEUE_CASE, 8
    tl = cc.TILES[tile]
    flags = dict(WPS_ENV_FLAGS)
    flags["reward_weights"] = dict(flags["reward_weights"], action=1.0, distance=0.5, s_quality=1.0)
    p = params_from_config(CASE_SPECS[case], flags, tile_agents=tl.A, tile_tasks=tl.T, tile_threats=tl.H)
    env = _handle(p, n)
    try:
        env.reset(np.arange(70, 70 + n, dtype=np.uint64))
        oracles = [orc.OracleEnv(p) for _ in range(n)]
        for i, o in enumerate(oracles):
            o.reset(70 + i)
        rng = np.random.default_rng(11)
        passed, compared = set(), 0
        for t in range(30):
            acts = []
            for i in range(n):
                items = []
                for a in rng.permutation(env.n_agents)[:int(rng.integers(1, 5))]:
                    # every other env draws from few distinct tasks: its queues stay short
                    items += [(int(a), int(rng.integers(0, 14 if i % 2 == 0 else 4))) for _ in range(int(rng.integers(1, 7)))]
                acts.append(items)
            aa, ai = env.pack_actions(acts)
            env.step(aa, ai)
            snap = Snapshot(env)
            for i, o in enumerate(oracles):
                if i in passed:
                    assert snap.ERROR[i] == cc.CODE["queue"]
                    continue
                o.step([a for a, _ in acts[i]], [j for _, j in acts[i]])
                if o.dims()["max_queue"] > tl.Q:
                    assert snap.ERROR[i] == cc.CODE["queue"], f"seed {70 + i} t={t + 1}: the oracle queues {o.dims()['max_queue']}, ERROR {snap.ERROR[i]}"
                    passed.add(i)
                else:
                    compare(snap, i, o, f"random lists seed {70 + i} t={t + 1}")
                    compared += 1
        assert 2 <= len(passed) < n and compared >= 60, f"{len(passed)} envs passed Q, {compared} comparisons"
    finally:
        env.close()
