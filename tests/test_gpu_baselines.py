"""Local-PI and Local-Cap-Greedy on the device (MUAVTA_ALLOC_PI / MUAVTA_ALLOC_CAP_GREEDY, csrc/sim/baselines.inc) against the host
restatement tests/baselines_py.py driving the facade over the CPU oracle, and against the reference's recorded episodes
(tests/golden/pi_* / capgreedy_*)."""
import glob
import os

import numpy as np
import pytest

import baselines_py as B
import orc
from oracle_backend import OracleBackend
from muavta_amd.env import MultiUAVEnv
from muavta_amd.params import METRIC_KEYS, params_for_case
from muavta_amd.scenarios import CASE_SPECS, WPS_ENV_FLAGS
from test_gpu_parity import Snapshot, compare

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
MODES = {"pi": "pi", "capgreedy": "cap_greedy"}


def _env(case, n, **kw):
    from muavta_amd.batched import BatchedMultiUAVEnv
    return BatchedMultiUAVEnv(params_for_case(case, **kw), n)


def _facade(case):
    return MultiUAVEnv(CASE_SPECS[case], backend=OracleBackend(params_for_case(case)), flags=dict(WPS_ENV_FLAGS))


def _host_metrics(facade, seed, mode, interval, use_vis=True):
    B.run_episode(facade, seed, mode, interval, use_vis)
    return facade._b.o.metrics().copy()


# 1. stepwise on every tile: env.allocate in each mode == baselines_py over the oracle facade, action for action, full state each step
@pytest.mark.parametrize("mode", ["pi", "cap_greedy"])
@pytest.mark.parametrize("case,interval,n", [("WPS_hard", 20, 3), ("WPS_escort24", 12, 2), ("WPS_burst64", 20, 2)])
def test_stepwise_vs_host(mode, case, interval, n):
    env = _env(case, n)
    assert {"WPS_hard": 16, "WPS_escort24": 24, "WPS_burst64": 64}[case] == env.A_tile
    env.set_allocator(mode)
    seeds = np.arange(n, dtype=np.uint64) + 3
    env.reset(seeds)
    facs = [_facade(case) for _ in range(n)]
    infos = [f.reset(seed=int(s))[1] for f, s in zip(facs, seeds)]
    pis = [B.PI(interval) for _ in range(n)]
    live = [True] * n
    tracked, compared = [True] * n, [0] * n  # (an env the tile flags is followed up to the step where the reference outgrows it)
    for t in range(150):
        if not any(live):
            break
        aa, ai = env.allocate(interval, True)
        for i, f in enumerate(facs):
            if not live[i]:
                continue
            if mode == "pi":
                acts, _ = B.pi_actions(f, pis[i], B.events_of(infos[i]), True)
            else:
                acts = B.cap_greedy_actions(f, True)
            want_a = [f.agent_by_name[nm].id for nm in acts]
            k = len(want_a)
            assert list(aa[i][:k]) == want_a and np.all(aa[i][k:] == -1), f"{mode} {case} env {i} t={t}: {aa[i]} vs {want_a}"
            assert list(ai[i][:k]) == list(acts.values()), f"{mode} {case} env {i} t={t}: indices"
            _, _, done, trunc, infos[i] = f.step(acts)
            live[i] = not (all(done.values()) or all(trunc.values()))
        env.step(aa, ai)
        snap = Snapshot(env)
        for i, f in enumerate(facs):
            if not tracked[i]:
                continue
            if snap.ERROR[i] == 2:  # MUAVTA_ERR_QUEUE: Cap-Greedy keeps queueing tasks on its best agent; the tile's queues are Q deep
                assert max(len(a.tasks) for a in f.agents_obj) > snap.AGENT_QUEUE.shape[2], f"{case} env {i} t={t + 1}: queue flag"
                tracked[i] = live[i] = False
                continue
            compared[i] += 1
            # N_REPLANS is the planner's counter: the host planner's here (the oracle's own counter belongs to its Hungarian planner)
            want_n = pis[i].n_replans if mode == "pi" else 0
            assert int(snap.SCALARS[i, 23]) == want_n, f"{case} env {i} t={t + 1}: n_replans {snap.SCALARS[i, 23]} vs {want_n}"
            snap.SCALARS[i, 23] = f._b.o.scalars()[23]
            compare(snap, i, f._b.o, f"{mode} {case} env {i} t={t + 1}")
    assert min(compared) >= 20, compared


# 2. the fused rollout reproduces the reference's metrics and n_replans; switching back to "hungarian" reproduces metrics_{case}
@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "pi_metrics_*.npz")) + glob.glob(os.path.join(GOLDEN, "capgreedy_metrics_*.npz"))),
                         ids=lambda p: os.path.basename(p)[:-4])
def test_fused_rollout_matches_reference(path):
    g = np.load(path)
    algo, case = os.path.basename(path)[:-4].split("_metrics_")
    want = g["metrics"]
    n = want.shape[0]
    env = _env(case, n)
    env.set_allocator(MODES[algo])
    seeds = np.arange(n, dtype=np.uint64)
    env.rollout(seeds, 150, int(g["interval"]), True, True)
    got, err = env.rollout_metrics(), env.get("ERROR").copy()
    reps = env.get("SCALARS")[:, 23].astype(int)
    # Cap-Greedy queues a task on its best agent at every step: some episodes outgrow a tile's task slots (code 1) or queue depth
    # (code 2).  Those are re-run on the 64 x 128 tile; what outgrows that too is flagged, never reported as a result.
    bad = np.nonzero(err)[0]
    assert set(err[bad].tolist()) <= {1, 2}, err[bad]
    if len(bad) and env.A_tile < 64:
        big = _env(case, len(bad), tile_agents=64, tile_tasks=128, tile_threats=48)
        big.set_allocator(MODES[algo])
        big.rollout(seeds[bad], 150, int(g["interval"]), True, True)
        bm, be, br = big.rollout_metrics(), big.get("ERROR"), big.get("SCALARS")[:, 23].astype(int)
        for k, i in enumerate(bad):
            if be[k] == 0:
                got[i], err[i], reps[i] = bm[k], 0, br[k]
    ok = err == 0
    assert ok.sum() >= max(4, n // 4), f"{algo} {case}: only {int(ok.sum())} of {n} episodes fit the tiles"
    assert np.array_equal(got[ok], want[ok]), f"{algo} {case}: seeds {np.nonzero(ok & ~np.all(got == want, axis=1))[0][:8]} differ"
    assert np.array_equal(reps[ok], g["n_replans"][ok])
    if algo == "pi":
        assert ok.all()
    env.set_allocator("hungarian")
    gm = np.load(os.path.join(GOLDEN, f"metrics_{case}.npz"))
    m = min(n, gm["metrics"].shape[0])
    env.rollout(np.arange(n, dtype=np.uint64), 150, int(gm["interval"]), True, False)
    assert np.array_equal(env.rollout_metrics()[:m], gm["metrics"][:m])


# 3. two seeded batches queued back to back on a two-lane handle == one-lane results; rollout_part with two parts == the whole batch
@pytest.mark.parametrize("mode", ["pi", "cap_greedy"])
def test_lanes_and_parts(mode):
    # (on the 24-agent tile: Cap-Greedy leaves tasks open long enough that a 16 x 40 batch of this size can hold an overflowing env)
    case, n, tile = "WPS_hard_x2", 64, dict(tile_agents=24, tile_tasks=48, tile_threats=24)
    sets = [np.arange(k * 1000, k * 1000 + n, dtype=np.uint64) for k in range(2)]
    one = _env(case, n, **tile)
    one.set_allocator(mode)
    one.set_lanes(1)
    want = []
    for sd in sets:
        one.rollout(sd, 150, 20, True, True)
        one.sync()
        want.append(one.rollout_metrics())
        assert not one.get("ERROR").any()
    two = _env(case, n, **tile)
    two.set_allocator(mode)
    two.set_lanes(2)
    for sd in sets:
        two.rollout(sd, 150, 20, True, True)  # no sync in between
    assert np.array_equal(two.rollout_metrics(back=1), want[0])
    assert np.array_equal(two.rollout_metrics(), want[1])
    parts = _env(case, n, **tile)
    parts.set_allocator(mode)
    parts.reset(sets[0])
    parts.set_parts(2)
    for p in range(2):
        parts.rollout_part(p, 150, 20, True, True)
    parts.sync()
    assert np.array_equal(parts.metrics(), want[0]) and not parts.get("ERROR").any()
    parts.set_parts(0)


# 4. rollout(escalate=True): an env that overflows the 16 x 40 tile gets the larger tile's row, equal to a direct rollout there
@pytest.mark.parametrize("mode", ["pi", "cap_greedy"])
def test_escalation_carries_the_mode(mode):
    case, n = "WPS_hard_x2", 64
    seeds = np.arange(500, 500 + n, dtype=np.uint64)
    small = _env(case, n)
    small.set_slot_cap(20)
    small.set_allocator(mode)
    small.rollout(seeds, 150, 20, True, True, escalate=True)
    assert len(small.escalated) > 0 and all(h.A_tile == 24 for h, _ in small.escalated.values())
    got = small.rollout_metrics()
    big = _env(case, n, tile_agents=24, tile_tasks=48, tile_threats=24)
    big.set_allocator(mode)
    big.rollout(seeds, 150, 20, True, True)
    direct = big.rollout_metrics()
    for i in small.escalated:
        assert np.array_equal(got[i], direct[i]), f"env {i}"
    ok = np.array([i not in small.escalated for i in range(n)])
    assert np.array_equal(got[ok], direct[ok])


# 5. random configurations of the wide fuzz generator: fused device rollout == baselines_py over the oracle, in both modes
def test_random_configs_fused_vs_host():
    from fuzz_device import tiles_for
    from fuzz_device_params import params_of_wide
    from fuzz_reference import wide_config
    from muavta_amd.batched import BatchedMultiUAVEnv

    checked = {"pi": 0, "cap_greedy": 0}
    k = 0
    while min(checked.values()) < 32 and k < 400:
        w = wide_config(k)
        k += 1
        cfg, interval, seed = w["cfg"], w["interval"], w["seed"]
        tiles = tiles_for(cfg)
        if not tiles:
            continue
        mode = "pi" if k % 2 else "cap_greedy"
        use_vis = k % 5 != 0
        p = params_of_wide(cfg, tiles[0])
        c = dict(cfg)
        c["threats_list"] = [tuple(x) for x in c["threats_list"]]
        c["escort_agent_types"] = tuple(c["escort_agent_types"])
        try:
            fac = MultiUAVEnv(c, backend=OracleBackend(params_of_wide(cfg, (64, 128, 48))), tile_agents=64, tile_tasks=128, tile_threats=48)
            want = _host_metrics(fac, seed, mode, interval, use_vis)
        except Exception as exc:  # a configuration the facade / oracle refuses (e.g. a queue deeper than the oracle exports)
            print(f"k={k - 1}: host skipped: {type(exc).__name__}: {exc}")
            continue
        env = BatchedMultiUAVEnv(p, 1)
        env.set_allocator(mode)
        env.rollout(np.array([seed], dtype=np.uint64), p.max_time_steps, interval, use_vis, k % 3 != 0)
        if env.get("ERROR")[0]:
            env.close()
            continue
        got = env.rollout_metrics()[0]
        env.close()
        assert np.array_equal(got, want), f"k={k - 1} {mode} tile {tiles[0]} seed {seed}: columns {np.nonzero(got != want)[0].tolist()}"
        checked[mode] += 1
    assert min(checked.values()) >= 32, checked


# 6. rollout_record refuses the baseline modes and the handle stays usable
@pytest.mark.parametrize("mode", ["pi", "cap_greedy"])
def test_rollout_record_refuses_baseline_modes(mode):
    import torch
    from muavta_amd.native import MuavtaError

    case, n, steps = "WPS_hard", 4, 20
    env = _env(case, n)
    env.set_allocator(mode)
    dev = torch.device("cuda", env.device_index)
    rings = {k: torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device=dev) for k, (shape, dt) in env.obs_ring_shapes(steps).items()}
    seeds = np.arange(n, dtype=np.uint64)
    with pytest.raises(MuavtaError, match="Cap-Greedy / PI"):
        env.rollout_record(seeds, steps, 20, True, obs_rings=rings)
    env.rollout(seeds, 150, 20, True, True)  # still usable, same results as a fresh handle
    fresh = _env(case, n)
    fresh.set_allocator(mode)
    fresh.rollout(seeds, 150, 20, True, True)
    assert np.array_equal(env.rollout_metrics(), fresh.rollout_metrics())
    env.set_allocator("hungarian")
    env.rollout_record(seeds, steps, 20, True, obs_rings=rings)
    env.sync()
