"""The device RNG across MT19937 block boundaries.  No 150-step episode of the registry draws 624 words from one stream
(test_rng_blocks_cpu.py records that), so these long-horizon configurations are what runs rng_refill_slow, the `off >= 624` reads of
next32 / rng_prefetch_issue, the block marker in rng_idx and its way through get_state / get_rng / set_state / set_rng.  Every (config,
seed) used here is guarded on the CPU by test_rng_blocks_cpu.py: the crossings (step, stream, offset, words) are the oracle's."""
import numpy as np
import pytest

import orc
import rng_blocks as rb
from test_gpu_parity import Snapshot, compare

pytestmark = pytest.mark.gpu


def _env(name, n):
    from muavta_amd.batched import BatchedMultiUAVEnv
    return BatchedMultiUAVEnv(rb.params(name), n)


def _oracles(name, seeds, n_steps):
    """One oracle per seed, advanced by reset + n_steps x (allocate -> step)."""
    out = []
    for s in seeds:
        o = orc.OracleEnv(rb.params(name))
        assert o.rollout(int(s), n_steps, rb.interval(name), 1) == n_steps
        out.append(o)
    return out


def _step_both(env, oracles, interval, tag):
    """One allocate -> step on the device and on every oracle, plans and every field compared."""
    aa, ai = env.allocate(interval, True)
    for i, o in enumerate(oracles):
        oa, oi = o.allocate(interval, 1)
        k = len(oa)
        assert np.array_equal(aa[i][:k], oa) and np.all(aa[i][k:] == -1) and np.array_equal(ai[i][:k], oi), f"{tag} env {i}: plan"
        o.step(oa, oi)
    env.step(aa, ai)
    snap = Snapshot(env)
    for i, o in enumerate(oracles):
        compare(snap, i, o, f"{tag} env {i}")


def _fields(env):
    """Every named state field plus the observation: the state as callers can read it."""
    out = {k: env.get(k) for k in Snapshot.NAMES}
    out.update(env.observe())
    return out


def _same_fields(a, b, tag):
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{tag}: {k}"


def _finish_and_compare(env, oracles, name, tag):
    """Fused rollout to the end of the episode; final state, observation and all 30 metrics against the oracles."""
    interval, left = rb.interval(name), rb.horizon(name) - oracles[0].dims()["time_steps"]
    env.rollout(None, left, interval, True, True)
    snap, m = Snapshot(env), env.metrics()
    for i, o in enumerate(oracles):
        o.rollout(0, left, interval, 1, do_reset=0)
        assert o.dims()["time_steps"] == rb.horizon(name) and o.dims()["truncated"]
        compare(snap, i, o, f"{tag} env {i} at the end")
        assert np.array_equal(m[i], o.metrics()), f"{tag} env {i}: final metrics"


WINDOWS, window_of = rb.WINDOWS, rb.window_of


@pytest.mark.parametrize("name,seeds,which", WINDOWS, ids=[f"{w[0]}-crossing{w[2]}" for w in WINDOWS])
def test_stepwise_around_each_crossing(name, seeds, which):
    """(a) The fused kernel up to three steps before the crossing, then allocate -> step with every field of every env compared after each
    step (the step that draws past word 624, the boundary after it that regenerates the block and flips the marker, and the draws
    from the new block), then the fused kernel to the end.  The second-crossing cases pass the first crossing inside the fused kernel."""
    first, last = window_of(name, seeds, which)
    assert 8 <= last - first <= 16
    env = _env(name, len(seeds))
    env.rollout(np.array(seeds, dtype=np.uint64), first, rb.interval(name), True, True)
    oracles = _oracles(name, seeds, first)
    snap = Snapshot(env)
    for i, o in enumerate(oracles):
        compare(snap, i, o, f"{name} seed {seeds[i]} after {first} fused steps")
    for t in range(first, last):
        _step_both(env, oracles, rb.interval(name), f"{name} seeds {seeds} t={t}")
    _finish_and_compare(env, oracles, name, f"{name} seeds {seeds}")


@pytest.mark.parametrize("name", list(rb.CONFIGS))
def test_fused_rollout_across_the_crossings_vs_oracle(name):
    """(b) One fused rollout of the whole long episode for 64 seeds: all 30 metrics of every env.  On the 700-step configurations the tgt
    stream of every seed crosses a block end twice; on the random-position one the agent stream of every seed crosses once, for
    more than half of the seeds inside the reset."""
    assert len(rb.FUSED_SEEDS[name]) == 64
    seeds = np.array(rb.FUSED_SEEDS[name], dtype=np.uint64)
    env = _env(name, len(seeds))
    env.rollout(seeds, rb.horizon(name), rb.interval(name), True, False)
    got, err = env.rollout_metrics(), env.get("ERROR")
    assert not err.any(), f"{name}: seeds {seeds[np.nonzero(err)[0]]} overflowed the tile (codes {np.unique(err[err != 0])})"
    assert np.all(env.get("SCALARS")[:, 0] == rb.horizon(name))
    want = orc.parallel_metrics(rb.params(name), seeds, rb.interval(name), n_steps=rb.horizon(name))
    bad = np.nonzero(~np.all(got == want, axis=1))[0]
    assert len(bad) == 0, f"{name}: seeds {seeds[bad[:8]]} differ"


def test_reset_that_crosses_a_block_end():
    """(c) The 64-agent random-position reset draws 588 .. 654 words from the agent stream of seeds 0..7 (620 for seed 0, which also draws 660
    from the tgt stream): past the 160-word reset window and, for five of the eight, past the end of block 0 with no regeneration in between.
    Every field after reset and after each of the first three steps; the first step boundary regenerates the block the reset consumed."""
    name, seeds = "burst64_random_init", list(range(8))
    env = _env(name, len(seeds))
    env.reset(np.array(seeds, dtype=np.uint64))
    oracles = _oracles(name, seeds, 0)
    snap = Snapshot(env)
    for i, o in enumerate(oracles):
        compare(snap, i, o, f"{name} seed {seeds[i]} after reset")
    for t in range(3):
        _step_both(env, oracles, rb.interval(name), f"{name} t={t}")


TAPE_SEEDS, TAPE_STOPS = rb.TAPE_SEEDS, rb.TAPE_STOPS


def _want_tapes(name, seeds, n_steps, streams):
    """The two tape halves of every (env, stream) after reset + n_steps steps: the device has regenerated a block at the start of
    every step that began with the cursor at or past word 624, so r = (words drawn before the last executed step) // 624 blocks are
    gone, the marker is r & 1, half [r & 1] holds block r and the other half block r + 1."""
    want = np.zeros((len(seeds), 4, 2, 624), dtype=np.uint32)
    for i, s in enumerate(seeds):
        words, _, _ = rb.trace(name, s, n_steps)
        assert len(words) == n_steps + 1
        ss = rb.stream_seeds(s)
        for st in streams:
            r = int(words[n_steps - 1, st]) // 624 if n_steps else 0
            blocks = rb.mt_blocks(ss[st], r + 2)
            want[i, st, r & 1] = blocks[r]
            want[i, st, (r & 1) ^ 1] = blocks[r + 1]
    return want


def test_tapes_after_reset_are_cpythons_first_two_blocks():
    """(d) get_rng() after reset against random.Random itself, not the oracle: k_seed (init_by_array with one- and two-word keys, the
    three randint(0, 2**63 - 1) stream seeds) and mt_twist_lds.  The obs stream is only seeded when the configuration has obstacles;
    without them its tape stays all zero (every step prefetches its next words into the state record, so it must not be stale memory)."""
    for name, streams in (("hard700", (rb.AGENT, rb.TGT, rb.MISSION)), ("burst64_random_init", (0, 1, 2, 3))):
        env = _env(name, len(TAPE_SEEDS))
        env.reset(np.array(TAPE_SEEDS, dtype=np.uint64))
        got, want = env.get_rng(), _want_tapes(name, TAPE_SEEDS, 0, streams)
        for i, s in enumerate(TAPE_SEEDS):
            for st in streams:
                assert np.array_equal(got[i, st, 0], want[i, st, 0]), f"{name} seed {s} stream {rb.STREAMS[st]}: block 0"
                assert np.array_equal(got[i, st, 1], want[i, st, 1]), f"{name} seed {s} stream {rb.STREAMS[st]}: block 1"
        if rb.OBS not in streams:  # never seeded: the tape a handle is created with is zero, not whatever the allocation held
            assert not got[:, rb.OBS].any(), f"{name}: the unseeded obs tape"


def test_tapes_after_each_crossing_are_cpythons_blocks_in_marker_order():
    """(d) After rollouts that end just after the first and just after the second crossing the two halves of every tape are CPython's
    raw blocks {k, k + 1}, in the order the marker implies: pins mt_twist (rng_refill_slow: phases, source / destination halves)
    without going through the simulation."""
    name, streams = "hard700", (rb.AGENT, rb.TGT, rb.MISSION)
    env = _env(name, len(TAPE_SEEDS))
    done = 0
    for stop in TAPE_STOPS:
        env.rollout(np.array(TAPE_SEEDS, dtype=np.uint64) if done == 0 else None, stop - done, rb.interval(name), True, False)
        done = stop
        assert not env.get("ERROR").any()
        got, want = env.get_rng(), _want_tapes(name, TAPE_SEEDS, stop, streams)
        for i, s in enumerate(TAPE_SEEDS):
            for st in streams:
                assert np.array_equal(got[i, st], want[i, st]), f"seed {s} stream {rb.STREAMS[st]} after {stop} steps"
    env = _env("burst64_random_init", 1)  # the block a RESET consumed (seed 0: agent at word 620, tgt at 660), regenerated by the first step
    env.rollout(np.zeros(1, dtype=np.uint64), 2, 20, True, False)
    assert np.array_equal(env.get_rng(), _want_tapes("burst64_random_init", [0], 2, (0, 1, 2, 3)))


def test_checkpoint_with_the_block_marker_set():
    """(e) Save at t = 400, where the tgt stream of every env has regenerated once (marker 1, between the two crossings); finish; scramble;
    restore into the same handle and into a fresh one; finish again: metrics and final state bit-equal, and equal to the oracle."""
    name, n, t_save = "hard700", 8, 400
    seeds, interval, left = np.arange(n, dtype=np.uint64), rb.interval(name), rb.horizon(name) - t_save
    env = _env(name, n)
    env.rollout(seeds, t_save, interval, True, True)
    state, rng = env.get_state(), env.get_rng()
    env.rollout(None, left, interval, True, True)
    m1, final1, rng1 = env.metrics(), _fields(env), env.get_rng()
    oracles = _oracles(name, seeds, rb.horizon(name))
    snap = Snapshot(env)
    for i, o in enumerate(oracles):
        compare(snap, i, o, f"seed {i} at the end")
        assert np.array_equal(m1[i], o.metrics()), f"seed {i}"
    env.rollout(seeds[::-1].copy() + np.uint64(100), 300, interval, True, True)  # scramble: other episodes, past their first crossing
    fresh = _env(name, n)
    for h, tag in ((env, "same handle"), (fresh, "fresh handle")):
        h.set_state(state); h.set_rng(rng)
        h.rollout(None, left, interval, True, True)
        assert np.array_equal(h.metrics(), m1) and np.array_equal(h.rollout_metrics(), m1), tag
        _same_fields(_fields(h), final1, tag)
        assert np.array_equal(h.get_rng(), rng1), tag


def test_step_run_across_the_crossing_vs_oracle():
    """(f) muavta_step_run (trainer gate, no step bound): for each of the four seeds the 20-step launches that start at t = 220 or 240 and at
    t = 540 run a crossing, the regeneration after it and the draws from the new block inside k_step_run's own loop.  Steps, park
    code and reward sum of every launch; every field of every env after the launches around both crossings; final state and metrics."""
    name, n, G = "hard700", 4, 1
    interval = rb.interval(name)
    env = _env(name, n)
    env.reset(np.arange(n, dtype=np.uint64))
    oracles = _oracles(name, range(n), 0)
    launches = 0
    while True:
        aa, ai = env.allocate(interval, True)
        t_before = [o.dims()["time_steps"] for o in oracles]
        nst, prk, rs = env.step_run(None, None, gate="trainer", replan_interval=interval, max_steps=0)
        near = any(200 <= t <= 260 or 520 <= t <= 580 for t in t_before)
        snap = Snapshot(env) if near else None
        for i, o in enumerate(oracles):
            oa, oi = o.allocate(interval, 1)  # (also for an env whose episode is over: the device planned for it too)
            k = len(oa)
            assert np.array_equal(aa[i][:k], oa) and np.all(aa[i][k:] == -1) and np.array_equal(ai[i][:k], oi), f"seed {i} launch {launches}: plan"
            d = o.dims()
            if d["terminated"] or d["truncated"]:
                assert nst[i] == 0 and (prk[i] & 3)
                continue
            o.step(oa, oi)
            q, ag, rq = o.run_quiet(G, interval, 0, 1, float(o.scalars()[1]))
            dd = o.dims()
            want_park = int(dd["terminated"]) | (int(dd["truncated"]) << 1) | (4 if ag else 0)
            assert int(nst[i]) == 1 + q and int(prk[i]) == want_park and rs[i] == rq, f"seed {i} launch {launches}: {nst[i]} {prk[i]} {rs[i]} vs {1 + q} {want_park} {rq}"
            if near:
                compare(snap, i, o, f"step_run seed {i} launch {launches}")
        launches += 1
        if np.all(prk & 3):
            break
        assert launches < 700
    snap, m = Snapshot(env), env.metrics()
    for i, o in enumerate(oracles):
        assert o.dims()["time_steps"] == rb.horizon(name)
        compare(snap, i, o, f"step_run seed {i} at the end")
        assert np.array_equal(m[i], o.metrics()), f"seed {i}: final metrics"


def test_rollout_by_two_parts_across_the_crossings_equals_the_whole_batch():
    """(f) rollout_part on two parts: launches that end before, on and after the crossing steps (the regeneration then falls on the first step
    of a launch or in the middle of one) end in the same state, tapes, observation and metrics as one rollout of the whole batch."""
    name, n = "hard700", 16
    seeds, interval = np.arange(n, dtype=np.uint64), rb.interval(name)
    ref = _env(name, n)
    ref.rollout(seeds, rb.horizon(name), interval, True, True)
    assert not ref.get("ERROR").any()
    env = _env(name, n)
    env.reset(seeds)
    env.set_parts(2)
    chunks = [228] + [1] * 16 + [296] + [3] * 6 + [142]  # single steps over 228 .. 243, threes over 540 .. 557
    assert sum(chunks) == rb.horizon(name)
    for k in chunks:
        for p in range(2):
            env.rollout_part(p, k, interval, True, True)
    got_obs, want_obs = env.observe(), ref.observe()
    assert np.array_equal(env.metrics(), ref.rollout_metrics()) and not env.get("ERROR").any()
    for key in want_obs:
        assert np.array_equal(got_obs[key], want_obs[key]), key
    env.set_parts(0)
    assert np.array_equal(env.get_state(), ref.get_state())  # (rng_win included: the prefetched words of all four streams)
    assert np.array_equal(env.get_rng(), ref.get_rng())


def test_two_lanes_back_to_back_rollouts_that_each_cross():
    """(f) Lanes mode 2: two seeded rollouts queued back to back land on the two lanes (each with its own tapes and cursors) and each crosses
    twice; both equal a one-lane handle that ran the batches one after the other, the latest one down to its tapes and (against the oracle) its state."""
    name, n = "hard700", 16
    interval, steps = rb.interval(name), rb.horizon(name)
    batches = [np.arange(n, dtype=np.uint64), np.arange(n, 2 * n, dtype=np.uint64)]
    env = _env(name, n)
    env.set_lanes(2)
    assert env.lanes() == (2, 2)
    env.rollout(batches[0], steps, interval, True, True)
    env.rollout(batches[1], steps, interval, True, True)
    got = [env.rollout_metrics(back=1), env.rollout_metrics()]
    assert not env.error_flags(back=1).any() and not env.error_flags().any()
    ref = _env(name, n)
    ref.set_lanes(1)
    for b in range(2):
        ref.rollout(batches[b], steps, interval, True, True)
        assert np.array_equal(got[b], ref.rollout_metrics()), f"batch {b}"
    assert np.array_equal(env.get_rng(), ref.get_rng())
    snap, snap_ref = Snapshot(env), Snapshot(ref)  # (slots of retired tasks keep what an earlier episode on that lane left: compare through the oracle)
    for i, o in enumerate(_oracles(name, batches[1], steps)):
        compare(snap, i, o, f"two lanes, seed {batches[1][i]}")
        compare(snap_ref, i, o, f"one lane, seed {batches[1][i]}")
        assert np.array_equal(got[1][i], o.metrics())
