"""Task.initTime / doneTime where the tile keeps them: in the LDS record on the 16-agent tile (TaskTimes in csrc/muavta_state.h), in the HBM
record on the 24- and 64-agent tiles.  Every reader of the two arrays goes through one accessor — the rebuild after an allocation changed,
both passes of the observation writer (columns 16 / 17: the full rows of a re-plan step, the light rows of every other step), task
creation, the release log, the host field reader — and each of them is compared here with the CPU oracle or with the same handle's own
earlier answer."""
import numpy as np
import pytest

import orc
from muavta_amd.params import params_for_case
from test_gpu_parity import Snapshot, compare

pytestmark = pytest.mark.gpu

CASE, INTERVAL, N, STEPS = "WPS_hard_x2", 20, 8, 60   # 16-agent tile, include_time_windows on
FUSED_STOPS = (21, 47, 60)                             # a re-plan step's full rows (21: the plan of t = 20), light rows, the end


def _env(case, n):
    from muavta_amd.batched import BatchedMultiUAVEnv
    return BatchedMultiUAVEnv(params_for_case(case), n)


def _oracles(case, n):
    out = [orc.OracleEnv(params_for_case(case)) for _ in range(n)]
    for i, o in enumerate(out):
        o.reset(i)
    return out


def _step_both(env, oracles, interval):
    aa, ai = env.allocate(interval, True)
    for i, o in enumerate(oracles):
        oa, oi = o.allocate(interval, 1)
        k = len(oa)
        assert np.array_equal(aa[i][:k], oa) and np.all(aa[i][k:] == -1) and np.array_equal(ai[i][:k], oi), f"env {i}: plan"
        o.step(oa, oi)
    env.step(aa, ai)
    return aa, ai


def _times_vs_oracle(env, oracles, tag):
    """TASK_TIMES of every open task and observation columns 16 / 17 against the oracle; returns (times, obs tasks)."""
    assert params_for_case(CASE).include_time_windows
    times, ids, obs = env.get("TASK_TIMES"), env.get("TASK_ID"), env.observe()["tasks"]
    for i, o in enumerate(oracles):
        trow, _ = o.tasks()
        for s in np.nonzero(ids[i] >= 0)[0]:
            k = int(ids[i, s])
            if int(trow[k, 0]) != 2:
                assert np.array_equal(times[i, s], trow[k, 3:5]), f"{tag} env {i}: task {k} init/done time"
        want = o.observe()[0]
        assert np.array_equal(obs[i][:, 16:18], want[:, 16:18]), f"{tag} env {i}: observation columns 16 / 17"
        assert np.array_equal(obs[i], want), f"{tag} env {i}: observation rows"
    return times, obs


@pytest.fixture(scope="module")
def stepwise():
    """The stepwise run, made once: per step the task times, the observation rows and the actions; the state + tapes at mid-episode."""
    env, oracles = _env(CASE, N), _oracles(CASE, N)
    env.reset(np.arange(N, dtype=np.uint64))
    rec = {"times": [], "obs": [], "acts": [], "ids": []}
    _times_vs_oracle(env, oracles, "after reset")
    rebuilt = light = 0
    prev = env.get("TASK_TIMES")
    for t in range(STEPS):
        if t == STEPS // 2:
            rec["state"], rec["rng"] = env.get_state(), env.get_rng()
        rec["acts"].append(_step_both(env, oracles, INTERVAL))
        times, obs = _times_vs_oracle(env, oracles, f"t={t + 1}")
        snap = Snapshot(env)
        for i, o in enumerate(oracles):
            compare(snap, i, o, f"{CASE} seed {i} t={t + 1}")
        changed = np.array([not np.array_equal(times[i], prev[i]) for i in range(N)])  # per env: the step rewrote some slot's times
        rebuilt, light, prev = rebuilt + int(changed.sum()), light + int((~changed).sum()), times
        rec["times"].append(times); rec["obs"].append(obs); rec["ids"].append(env.get("TASK_ID"))
    # (not vacuous: every env re-plans at t = 0, 20, 40; and at least one step in eight of an env neither creates a task nor changes a queue)
    assert rebuilt >= 3 * N and light >= N * STEPS // 8, f"(env, step) pairs that rewrote the times: {rebuilt}, that only read them: {light}"
    rec["final"] = {k: env.get(k) for k in Snapshot.NAMES}
    return rec


def test_task_times_and_observation_columns_stepwise_vs_oracle(stepwise):
    """60 x (allocate -> step): TASK_TIMES, columns 16 / 17 and every other field after every step (asserted while the fixture runs);
    the run has steps that rebuild the times and steps whose light rows only read them."""
    assert len(stepwise["times"]) == STEPS


def test_fused_rollout_equals_the_stepwise_run(stepwise):
    """The fused rollout stopped after a re-plan step, in a run of light steps and at the end: times, rows and fields of the stepwise run."""
    for stop in FUSED_STOPS:
        env = _env(CASE, N)
        env.rollout(np.arange(N, dtype=np.uint64), stop, INTERVAL, True, True)
        live = stepwise["ids"][stop - 1] >= 0
        assert np.array_equal(env.get("TASK_ID"), stepwise["ids"][stop - 1]), f"fused {stop}: slots"
        assert np.array_equal(env.get("TASK_TIMES")[live], stepwise["times"][stop - 1][live]), f"fused {stop}: TASK_TIMES"
        assert np.array_equal(env.observe()["tasks"], stepwise["obs"][stop - 1]), f"fused {stop}: observation rows"
    for k in Snapshot.NAMES:
        if k not in ("TASK_TIMES", "TASK_CUR", "TASK_ALLOC", "TASK_ORG_DONE", "TASK_POS", "TASK_META", "TASK_STATUS", "KNOWN"):  # (per-slot fields: free slots keep leftovers)
            assert np.array_equal(env.get(k), stepwise["final"][k]), f"fused {STEPS}: {k}"


def test_state_round_trip_mid_episode(stepwise):
    """get_state / get_rng at t = 30 restored into a fresh handle: the field reader returns the same times at once, the recorded actions
    lead through the same times and rows as the uninterrupted run, and a TASK_TIMES written through muavta_set is read back."""
    env = _env(CASE, N)
    env.set_state(stepwise["state"]); env.set_rng(stepwise["rng"])
    assert np.array_equal(env.get("TASK_TIMES"), stepwise["times"][STEPS // 2 - 1])
    for t in range(STEPS // 2, STEPS):
        aa, ai = env.allocate(INTERVAL, True)
        assert np.array_equal(aa, stepwise["acts"][t][0]) and np.array_equal(ai, stepwise["acts"][t][1]), f"t={t}: plan"
        env.step(aa, ai)
        assert np.array_equal(env.get("TASK_TIMES"), stepwise["times"][t]), f"t={t + 1}: TASK_TIMES"
        assert np.array_equal(env.observe()["tasks"], stepwise["obs"][t]), f"t={t + 1}: observation rows"
    mine = np.arange(env.get("TASK_TIMES").size, dtype=np.float64).reshape(env.get("TASK_TIMES").shape) + 0.25
    env.set("TASK_TIMES", mine)
    assert np.array_equal(env.get("TASK_TIMES"), mine)
    other = _env(CASE, N)
    other.set_state(env.get_state())
    assert np.array_equal(other.get("TASK_TIMES"), mine)


def test_refresh_observation_keeps_the_rebuilt_times_in_the_record():
    """A fused rollout without the per-step observation write leaves the times to be rebuilt; muavta_refresh_observation rebuilds them and
    clears the flag, so the record it leaves must hold them: the field reader and the light rows of the next steps read them from there."""
    env, oracles = _env(CASE, N), _oracles(CASE, N)
    env.rollout(np.arange(N, dtype=np.uint64), 45, INTERVAL, True, False)
    for i, o in enumerate(oracles):
        assert o.rollout(i, 45, INTERVAL, 1) == 45
    env.refresh_observation()
    _times_vs_oracle(env, oracles, "after refresh_observation")
    for t in range(45, 50):
        _step_both(env, oracles, INTERVAL)
        _times_vs_oracle(env, oracles, f"t={t + 1}")


def test_release_log_rows_carry_the_times_the_slot_held():
    """The release log row of a task that leaves the device holds the slot's initTime / doneTime as they stood: a retired slot is not
    rebuilt any more, so they are what the field reader returned for that id after the step before (-1, -1 for a task born in this step)."""
    n = 4
    env, oracles = _env(CASE, n), _oracles(CASE, n)
    env.set_release_log(True)
    env.reset(np.arange(n, dtype=np.uint64))
    T = env.get("TASK_ID").shape[1]
    rows_seen = with_times = 0
    for t in range(150):
        ids, times = env.get("TASK_ID"), env.get("TASK_TIMES")
        _step_both(env, oracles, INTERVAL)
        log = env.get("RELEASE_LOG")
        for i in range(n):
            cnt = int(log[i, :1].view(np.int32)[0])
            assert 0 <= cnt <= T
            for r in log[i, 1:1 + 29 * cnt].reshape(cnt, 29):
                at = np.nonzero(ids[i] == int(r[0]))[0]
                want = times[i, at[0]] if len(at) else np.array([-1.0, -1.0])
                assert np.array_equal(r[15:17], want), f"t={t} env {i}: released task {int(r[0])}"
                rows_seen += 1
                with_times += bool(r[15] >= 0)
    assert rows_seen >= 1 and with_times >= 1, f"{rows_seen} release rows, {with_times} of them with an initTime"  # (not vacuous)


@pytest.mark.parametrize("case,interval,n", [("WPS_escort24", 12, 3), ("WPS_burst64", 20, 2)], ids=["tile24", "tile64"])
def test_tiles_that_keep_the_times_in_the_hbm_record(case, interval, n):
    """The 24- and 64-agent tiles keep the two arrays in the HBM record: every field and the observation after each of 40 steps."""
    from muavta_amd.batched import BatchedMultiUAVEnv
    env = BatchedMultiUAVEnv(params_for_case(case), n)
    oracles = _oracles(case, n)
    env.reset(np.arange(n, dtype=np.uint64))
    for t in range(40):
        _step_both(env, oracles, interval)
        snap = Snapshot(env)
        for i, o in enumerate(oracles):
            compare(snap, i, o, f"{case} seed {i} t={t + 1}")
