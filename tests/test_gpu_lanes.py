"""State lanes (muavta_set_lanes) against one lane: include/muavta.h promises that a handle running its seeded rollouts on two lanes
returns what the same calls return on one lane, bit for bit.  These tests queue the calls whose ordering the lanes change — recording
rollouts, waits on a caller's stream, settings made before the second lane exists, the pipeline's failed batch — and compare every
output with a set_lanes(1) handle given the same calls (and with the oracle where it has the mode).  Every comparison is exact.

A mode-0 flip depends on timing (the previous rollout must still be running when the next seeded call checks it), so the tests that
need one make it certain: a torch stream sleeps (`Hold`), the handle waits on that stream, and the rollout queued behind the wait
cannot finish before the sleep does.  Each hold is measured and asserted to last at least 10x the one-lane duration of the launch it
must cover, and each such test asserts that the flip happened."""
import numpy as np
import pytest

import orc
from muavta_amd.params import params_for_case
from test_gpu_parity import Snapshot, compare

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A  # byte pattern of the "torch still uses this block" fill: no ring element can hold it in every byte


def _env(case, n, lanes=None, **kw):
    from muavta_amd.batched import BatchedMultiUAVEnv
    e = BatchedMultiUAVEnv(params_for_case(case, **kw), n)
    if lanes is not None:
        e.set_lanes(lanes)
    return e


def _alloc(shapes, dev):
    import torch
    return {k: torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device=dev) for k, (shape, dt) in shapes.items()}


def _rings(env, steps, kind="pair", mt=32, ma=16):
    """(token rings, observation rings) of one rollout_record call, zero-filled (the fills are complete when this returns)"""
    import torch
    dev = torch.device("cuda", env.device_index)
    tok, obs = _alloc(env.record_shapes(kind, steps, mt, ma), dev), _alloc(env.obs_ring_shapes(steps), dev)
    torch.cuda.synchronize()
    return tok, obs


def _host(rings):
    return {k: v.cpu().numpy() for k, v in rings.items()}


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _assert_rings_equal(got, want, tag):
    assert got.keys() == want.keys()
    for k in want:
        g, w = got[k], want[k]
        if not _same_bytes(g, w):
            diff = (np.ascontiguousarray(g).view(np.uint8) != np.ascontiguousarray(w).view(np.uint8)).reshape(g.shape[0], -1).any(axis=1)
            raise AssertionError(f"{tag}: ring {k} differs from the one-lane handle's in slots {np.nonzero(diff)[0][:10].tolist()}")


def _sentinels(a):
    """elements of `a` still holding the sentinel in every byte"""
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1, a.itemsize)
    return int((b == SENTINEL).all(axis=1).sum())


def _assert_no_sentinel(rings, tag):
    left = {k: _sentinels(v) for k, v in rings.items()}
    assert not any(left.values()), f"{tag}: sentinel found in {[(k, c) for k, c in left.items() if c]}"


def _assert_unwritten_after_end(done, tag):
    """obs_done [n_steps, N]: slots up to and including an env's last step hold its done bits, every later one MUAVTA_OBS_UNWRITTEN"""
    from muavta_amd.batched import BatchedMultiUAVEnv
    U = BatchedMultiUAVEnv.OBS_UNWRITTEN
    K, N = done.shape
    for i in range(N):
        col = done[:, i]
        ended = np.nonzero((col != U) & ((col & 3) != 0))[0]
        t_end = int(ended[0]) + 1 if len(ended) else K
        assert np.all(col[:t_end] != U) and np.all(col[:t_end] <= 3), f"{tag}: env {i}: {int(np.count_nonzero(col[:t_end] == U))} of its {t_end} written obs_done slots read 0x80"
        assert np.all(col[t_end:] == U), f"{tag}: env {i}: slots after its last step ({t_end}) are not MUAVTA_OBS_UNWRITTEN"


def _obs_rings_vs_oracle(case, seed, R, i, steps, interval, MT):
    """slot t of the observation rings of env i = what the oracle's DroneEnv.step returns at step t (as
    test_observation_rings_of_the_fused_rollout_vs_oracle checks it)"""
    o = orc.OracleEnv(params_for_case(case))
    o.reset(int(seed))
    t_end = steps
    for t in range(steps):
        a, ix = o.allocate_mode(interval, 1, 0)
        o.step(a, ix)
        ti, legal, pad, ag, fl = o.observe()
        tag = f"{case} seed {seed} ring slot {t}"
        assert np.array_equal(R["obs_tasks"][t, i].T, ti), f"{tag}: tasks_info"
        bits = ((R["obs_legal"][t, i][:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(legal.shape[0], -1)[:, :MT]
        assert np.array_equal(bits.astype(bool), legal), f"{tag}: legal_mask"
        assert np.array_equal(R["obs_pad"][t, i].astype(bool), pad), f"{tag}: pad mask"
        assert np.array_equal(R["obs_agents"][t, i], ag), f"{tag}: agent rows"
        assert np.array_equal(R["obs_flags"][t, i], fl), f"{tag}: event flags"
        d = o.dims()
        assert R["obs_reward"][t, i] == o.scalars()[1], f"{tag}: reward"
        assert R["obs_done"][t, i] == (1 if d["terminated"] else 0) | (2 if d["truncated"] else 0), f"{tag}: done flags"
        if d["terminated"] or d["truncated"]:
            t_end = t + 1
            break
    assert np.all(R["obs_done"][t_end:, i] == 0x80), f"{case} seed {seed}: slots after the last step"
    return o


class Hold:
    """A torch stream that sleeps: work a handle queues after `env.wait_stream(hold.s)` cannot start before the sleep ends.
    Calibrated once: one timed sleep gives the cycles per ms, and the hold is sized to 15x `cover_ms` (the one-lane duration of
    the launch it must cover).  `check()` asserts, from the hold's own events, that it lasted at least 10x `cover_ms` and under 1 s."""
    CAL_CYCLES = 2_000_000

    def __init__(self, cover_ms):
        import torch
        self.torch = torch
        self.cover_ms = float(cover_ms)
        assert self.cover_ms > 0
        self.s = torch.cuda.Stream()
        self.s.wait_stream(torch.cuda.current_stream())
        per_ms = 0.0
        for _ in range(2):  # (the first sleep also pays for loading the kernel)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(self.s):
                a.record()
                torch.cuda._sleep(self.CAL_CYCLES)
                b.record()
            b.synchronize()
            per_ms = self.CAL_CYCLES / a.elapsed_time(b)
        self.cycles = int(per_ms * 15.0 * self.cover_ms) + 1
        assert 15.0 * self.cover_ms < 700.0, f"the launch to cover takes {self.cover_ms:.1f} ms: a hold of 15x that is not well under 1 s"
        self.ev = None

    def start(self):
        """queue the sleep on `s` (and return `s`, e.g. to queue the consumer's work behind it)"""
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.s):
            a.record()
            torch.cuda._sleep(self.cycles)
            b.record()
        self.ev = (a, b)
        return self.s

    def check(self):
        a, b = self.ev
        b.synchronize()
        ms = a.elapsed_time(b)
        print(f"hold {ms:.2f} ms for a {self.cover_ms:.2f} ms launch")
        assert ms >= 10.0 * self.cover_ms, f"hold of {ms:.2f} ms < 10 x {self.cover_ms:.2f} ms: the test did not hold the lane long enough"
        assert ms < 1000.0, f"hold of {ms:.2f} ms"
        return ms


TASK_SLOT_FIELDS = ("TASK_POS", "TASK_CUR", "TASK_ALLOC", "TASK_ORG_DONE", "TASK_META", "TASK_TIMES")


def _assert_same_env_state(sa, sb, tag):
    """every device field of every env equal, read as compare() reads the state against the oracle: the task-slot fields in the live
    slots (TASK_ID >= 0, equal first), the threats that exist, the drained events.  A free slot keeps whatever an earlier batch of its
    lane left there, and two lanes have different earlier batches."""
    for name in Snapshot.NAMES:
        a, b = getattr(sa, name), getattr(sb, name)
        if name in TASK_SLOT_FIELDS:
            live = sa.TASK_ID >= 0
            a, b = a[live], b[live]
        elif name in ("THREAT_POS", "THREAT_META"):
            assert np.array_equal(sa.THREAT_META[..., 0], sb.THREAT_META[..., 0]), f"{tag}: threat status"
            act = sa.THREAT_META[..., 0] != -9
            a, b = a[act], b[act]
        elif name == "EVENTS":
            assert np.array_equal(sa.EVENTS[..., 0] >= 0, sb.EVENTS[..., 0] >= 0), f"{tag}: drained event count"
            ev = sa.EVENTS[..., 0] >= 0
            a, b = a[ev], b[ev]
        if not np.array_equal(a, b):
            raise AssertionError(f"{tag}: {name} differs from the one-lane handle's")


# 1. two recording rollouts queued back to back in mode 2: the second (short) one ends long before the first (long) one
REC_CASES = [("WPS_hard_x2", 20, 256), ("WPS_escort24", 12, 128), ("WPS_burst64", 20, 64)]


@pytest.mark.parametrize("case,interval,n", REC_CASES, ids=[c[0] for c in REC_CASES])
def test_two_recording_rollouts_queued_back_to_back_in_mode_2(case, interval, n):
    long_steps, short_steps = 150, 8
    seeds1 = np.arange(70, 70 + n, dtype=np.uint64)
    seeds2 = np.arange(40000, 40000 + n, dtype=np.uint64)
    env = _env(case, n, lanes=2)
    ref = _env(case, n, lanes=1)
    got = [_rings(env, long_steps), _rings(env, short_steps)]
    want = [_rings(ref, long_steps), _rings(ref, short_steps)]
    # one lane: the same two calls
    ref.rollout_record(seeds1, long_steps, interval, True, want[0][0], "pair", 32, 16, obs_rings=want[0][1])
    ref.sync()
    m1 = ref.rollout_metrics()
    ref.rollout_record(seeds2, short_steps, interval, True, want[1][0], "pair", 32, 16, obs_rings=want[1][1])
    ref.sync()
    m2 = ref.rollout_metrics()
    # two lanes, nothing in between: call 2 runs on the other lane next to call 1
    env.rollout_record(seeds1, long_steps, interval, True, got[0][0], "pair", 32, 16, obs_rings=got[0][1])
    env.rollout_record(seeds2, short_steps, interval, True, got[1][0], "pair", 32, 16, obs_rings=got[1][1])
    env.sync()
    assert env.lanes() == (2, 2)
    ms = env.kernel_ms_history(2)
    print(f"{case}: launch 1 {ms[0]:.2f} ms, launch 2 {ms[1]:.2f} ms")
    assert ms[0] >= 4.0 * ms[1], f"{case}: launch 1 ({ms[0]:.2f} ms) was expected to last at least 4x launch 2 ({ms[1]:.2f} ms)"
    for k, (steps, tag) in enumerate(((long_steps, "call 1"), (short_steps, "call 2"))):
        g_tok, g_obs = _host(got[k][0]), _host(got[k][1])
        w_tok, w_obs = _host(want[k][0]), _host(want[k][1])
        _assert_unwritten_after_end(g_obs["obs_done"], f"{case} {tag}")
        _assert_rings_equal(g_obs, w_obs, f"{case} {tag}")
        _assert_rings_equal(g_tok, w_tok, f"{case} {tag}")
        if k == 0:
            for i in (0, n - 1):
                _obs_rings_vs_oracle(case, seeds1[i], g_obs, i, steps, interval, env.max_tasks)
    assert np.array_equal(env.rollout_metrics(back=1), m1)
    assert np.array_equal(env.rollout_metrics(), m2)
    assert not env.get("ERROR").any()


# 2. a forced mode-0 flip while a torch consumer still uses the rings: the new lane waits for it
def _fill_sentinel(hold_stream, ring_sets):
    import torch
    with torch.cuda.stream(hold_stream):  # (queued on the hold's stream, behind the sleep: "torch still uses the blocks")
        for rings in ring_sets:
            for t in rings.values():
                t.view(torch.uint8).fill_(SENTINEL)


@pytest.mark.parametrize("variant", ["rollout_record", "il_record", "set_lanes_after_wait"])
def test_forced_flip_waits_for_the_torch_consumer(variant):
    import torch
    from muavta_amd.il import il_record

    case, interval, n, steps = "WPS_hard_x2", 20, 64, 150
    seeds_a = np.arange(500, 500 + n, dtype=np.uint64)
    seeds_b = np.arange(7000, 7000 + n, dtype=np.uint64)
    env = _env(case, n)
    ref = _env(case, n, lanes=1)
    assert env.lanes() == (0, 1)
    tok, obs = _rings(env, steps)
    rtok, robs = _rings(ref, steps)
    # one lane: the same calls
    ma = None
    if variant != "set_lanes_after_wait":
        ref.rollout(seeds_a, steps, interval, True, True)
        ref.sync()
        ma = ref.rollout_metrics()
    if variant == "il_record":
        want = il_record(ref, seeds_b, steps, interval, "pair", 32, 16, rings=rtok)
        want = {k: v.cpu().numpy() for k, v in want.items()}
    else:
        ref.rollout_record(seeds_b, steps, interval, True, rtok, "pair", 32, 16, obs_rings=robs)
        ref.sync()
        want = {**_host(rtok), **_host(robs)}
    mb = ref.rollout_metrics()
    hold = Hold(float(ref.kernel_ms_history(2).max()) if ma is not None else ref.last_kernel_ms())
    s = hold.start()
    if variant == "set_lanes_after_wait":
        _fill_sentinel(s, (tok, obs))
        env.wait_stream(s.cuda_stream)
        env.set_lanes(2)  # the second lane is created after the wait
        env.rollout_record(seeds_b, steps, interval, True, tok, "pair", 32, 16, obs_rings=obs)
        assert env.lanes() == (2, 2)
    else:
        env.wait_stream(s.cuda_stream)
        env.rollout(seeds_a, steps, interval, True, True)  # cannot finish before the hold does
        if variant == "il_record":
            _fill_sentinel(s, (tok,))
            with torch.cuda.stream(s):
                out = il_record(env, seeds_b, steps, interval, "pair", 32, 16, rings=tok)  # wait_stream(torch's current stream = s); record
        else:
            _fill_sentinel(s, (tok, obs))
            env.wait_stream(s.cuda_stream)
            env.rollout_record(seeds_b, steps, interval, True, tok, "pair", 32, 16, obs_rings=obs)
        assert env.lanes() == (0, 2), "the seeded call was expected to find the held rollout unfinished and flip"
    env.sync()
    torch.cuda.synchronize()
    hold.check()
    if variant == "il_record":
        got = {k: v.cpu().numpy() for k, v in out.items()}
    else:
        got = {**_host(tok), **_host(obs)}
    _assert_no_sentinel(got, f"{variant}")
    if "obs_done" in got:
        _assert_unwritten_after_end(got["obs_done"], variant)
    _assert_rings_equal(got, want, variant)
    assert np.array_equal(env.rollout_metrics(), mb)
    if variant != "il_record":  # (il_record's expert is pinned to the reference by test_gpu_parity; here the one-lane handle is the yardstick)
        o = _obs_rings_vs_oracle(case, seeds_b[0], got, 0, steps, interval, env.max_tasks)
        compare(Snapshot(env), 0, o, f"{variant}: env 0 after the recorded rollout")
    if ma is not None:
        assert np.array_equal(env.rollout_metrics(back=1), ma)


# 3. settings made before the second lane exists are carried onto it; settings changed later reach both lanes
ESC_IV = {"hungarian": 12, "urgency_coalition": 12, "pi": 12, "cap_greedy": 12}
LANE_TILES = [("WPS_escort24", {}, 64, 11, 8),  # (its own 24 x 48 tile)
              ("WPS_escort24", dict(tile_agents=64, tile_tasks=128, tile_threats=48), 32, 50011, 2)]
ORACLE_MODE = {"hungarian": 0, "urgency_coalition": 2}


def _check_batch(case, seeds, mode, interval, got, flags, want, want_flags, n_host, tag):
    """one batch: bit-equal to the one-lane handle; unflagged envs (at least 3/4 of them) equal the oracle's rollout_mode, or for the
    two baselines the oracle has no mode for, the host restatement tests/baselines_py.py (the yardstick test_gpu_baselines uses)"""
    n = len(seeds)
    assert np.array_equal(flags, want_flags), f"{tag}: capacity flags"
    assert np.array_equal(got, want), f"{tag}: rows {np.nonzero(~np.all(got == want, axis=1))[0][:8]} differ from the one-lane handle"
    ok = flags == 0
    print(f"{tag}: {int(ok.sum())} of {n} envs unflagged")
    assert 4 * int(ok.sum()) >= 3 * n, f"{tag}: only {int(ok.sum())} of {n} envs fit the tile"
    if mode in ORACLE_MODE:
        o = orc.parallel_metrics(case, seeds, interval, 1, ORACLE_MODE[mode])
        assert np.array_equal(got[ok], o[ok]), f"{tag}: rows {np.nonzero(ok & ~np.all(got == o, axis=1))[0][:8]} differ from the oracle"
    else:
        from test_gpu_baselines import _facade, _host_metrics
        fac = _facade(case)
        for i in np.nonzero(ok)[0][:n_host]:
            assert np.array_equal(got[i], _host_metrics(fac, int(seeds[i]), mode, interval)), f"{tag}: env {i} vs the host restatement"


@pytest.mark.parametrize("case,tile,n,seed0,n_host", LANE_TILES, ids=["tile24x48", "tile64x128"])
def test_settings_reach_the_second_lane_before_and_after_it_exists(case, tile, n, seed0, n_host):
    """(The oracle restates Hungarian and Urgency-Coalition only: Local-PI and Local-Cap-Greedy rows are checked against the host
    restatement for n_host envs per batch — a whole host episode on the 24-agent workload takes seconds — and, every env, against
    the one-lane handle, whose fused baseline rollouts test_gpu_baselines pins to the reference.)"""
    import torch

    modes = ["hungarian", "urgency_coalition", "pi", "cap_greedy"]
    intervals = ESC_IV
    batches = [np.arange(3000 * b + seed0, 3000 * b + seed0 + n, dtype=np.uint64) for b in range(len(modes))]
    env = _env(case, n, **tile)
    ref = _env(case, n, lanes=1, **tile)
    for e in (env, ref):  # before any flip: the twin does not exist yet
        e.set_allocator(modes[0])
        e.set_parts(2)
        e.set_release_log(True)
    # one lane: every batch with its allocator
    want, want_flags, ms0 = [], [], None
    for b, seeds in enumerate(batches):
        ref.set_allocator(modes[b])
        ref.rollout(seeds, 150, intervals[modes[b]], True, True)
        ref.sync()
        if b == 0:
            ms0 = ref.last_kernel_ms()
        want.append(ref.rollout_metrics())
        want_flags.append(ref.get("ERROR"))
    hold = Hold(ms0)
    got, flags = [None] * len(batches), [None] * len(batches)
    s = hold.start()
    env.wait_stream(s.cuda_stream)
    env.rollout(batches[0], 150, intervals[modes[0]], True, True)  # held: still running at the next seeded call
    env.set_allocator(modes[1])  # still one lane: the twin must take it over when it is created
    env.rollout(batches[1], 150, intervals[modes[1]], True, True)
    assert env.lanes() == (0, 2), "the seeded call was expected to find the held rollout unfinished and flip"
    got[0], flags[0] = env.rollout_metrics(back=1), env.error_flags(back=1)
    hold.check()
    env.set_lanes(2)  # continue alternating; the allocator changes below reach both lanes
    for b in (2, 3):
        env.set_allocator(modes[b])
        env.rollout(batches[b], 150, intervals[modes[b]], True, True)
        got[b - 1], flags[b - 1] = env.rollout_metrics(back=1), env.error_flags(back=1)
    got[3], flags[3] = env.rollout_metrics(), env.error_flags()
    assert env.lanes() == (2, 2)
    for b, seeds in enumerate(batches):
        _check_batch(case, seeds, modes[b], intervals[modes[b]], got[b], flags[b], want[b], want_flags[b], n_host, f"{case} tile {env.A_tile}x{env.T} batch {b} ({modes[b]})")
    # after the last flip every entry point works on the latest lane, as on one lane
    iv = intervals["hungarian"]
    tail = np.arange(90000, 90000 + n, dtype=np.uint64)
    for e in (env, ref):
        e.set_allocator("hungarian")
        e.set_release_log(False)  # (the release log is a whole-batch facility: step_part refuses it)
        e.rollout(tail, 40, iv, True, True)
    assert env.lanes() == (2, 2)
    for e in (env, ref):
        for p in range(2):
            e.rollout_part(p, 10, iv, True, True)
        e.sync()
    for p in range(2):
        ga, gi = env.allocate_part(p, iv, True)
        wa, wi = ref.allocate_part(p, iv, True)
        assert np.array_equal(ga, wa) and np.array_equal(gi, wi), f"allocate_part {p}"
        env.step_part(p)
        ref.step_part(p)
    for e in (env, ref):
        e.sync()
        e.allocate(iv, True, fetch=False)
    for x, y in zip(env.step_run(None, None, "trainer", iv, 6, True), ref.step_run(None, None, "trainer", iv, 6, True)):
        assert np.array_equal(x, y), "step_run"
    dev = torch.device("cuda", env.device_index)
    tg, tw = _alloc(env.token_shapes("pair", 32, 16), dev), _alloc(ref.token_shapes("pair", 32, 16), dev)
    cg, cw = torch.zeros((n, 8), dtype=torch.float32, device=dev), torch.zeros((n, 8), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    env.tokens("pair", 32, 16, out=tg); ref.tokens("pair", 32, 16, out=tw)
    env.context("pair", 32, out=cg); ref.context("pair", 32, out=cw)
    env.sync(); ref.sync()
    _assert_rings_equal(_host(tg), _host(tw), "tokens(out=...)")
    assert _same_bytes(cg.cpu().numpy(), cw.cpu().numpy()), "context(out=...)"
    oa, ob = env.observe(), ref.observe()
    assert all(_same_bytes(oa[k], ob[k]) for k in ob), "observe"
    assert np.array_equal(env.metrics(), ref.metrics())
    _assert_same_env_state(Snapshot(env), Snapshot(ref), f"{case} after the last flip")


# 4. the pipeline survives a failed batch
def test_in_flight_pipeline_survives_a_failed_batch():
    from muavta_amd.native import MuavtaError
    from muavta_amd.pipeline import InFlightRollouts

    case, n, cap, interval = "WPS_hard_x2", 8, 20, 20  # (the cap test_escalation_carries_the_mode uses)
    scan = _env(case, 1024, lanes=1)
    scan.set_slot_cap(cap)
    scan.rollout(np.arange(1024, dtype=np.uint64), 150, interval, True, True)
    flagged = scan.get("ERROR") != 0
    clean, dirty = np.nonzero(~flagged)[0], np.nonzero(flagged)[0]
    print(f"seed scan at slot cap {cap}: {len(clean)} clean, {len(dirty)} flagged of 1024")
    assert len(clean) >= 4 * n and len(dirty) >= 1, "the seed scan was expected to find clean seeds and a flagged one"
    bad = np.concatenate([clean[3 * n:4 * n - 1], dirty[:1]])  # one flagged env among clean ones
    batches = [clean[:n], bad, clean[n:2 * n], clean[2 * n:3 * n]]
    batches = [np.ascontiguousarray(b, dtype=np.uint64) for b in batches]
    one = _env(case, n, lanes=1)
    one.set_slot_cap(cap)
    want = []
    for k, seeds in enumerate(batches):
        one.rollout(seeds, 150, interval, True, True)
        want.append(one.rollout_metrics())
        assert np.array_equal(one.error_flags() != 0, np.arange(n) == (n - 1 if k == 1 else n)), f"batch {k}: flags of the one-lane run"
    pipe = InFlightRollouts(params_for_case(case), n)
    pipe.envs[0].set_slot_cap(cap)
    pipe.submit(batches[0], 150, interval, tag="clean0")
    pipe.submit(batches[1], 150, interval, tag="bad")
    tag, m = next(pipe.results())
    assert tag == "clean0" and np.array_equal(m, want[0])
    pipe.submit(batches[2], 150, interval, tag="clean1")
    with pytest.raises(MuavtaError) as ei:
        next(pipe.results())
    assert ei.value.tag == "bad" and np.array_equal(ei.value.metrics, want[1])
    assert np.array_equal(ei.value.error_flags != 0, np.arange(n) == n - 1)
    pipe.submit(batches[3], 150, interval, tag="clean2")  # the failed batch left the queue: room again
    got = list(pipe.results(all_pending=True))
    assert [t for t, _ in got] == ["clean1", "clean2"]
    assert np.array_equal(got[0][1], want[2]) and np.array_equal(got[1][1], want[3])
    assert pipe.envs[0].lanes() == (2, 2)
    pipe.close()
