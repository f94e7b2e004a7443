"""step() walks the live task slots once (Sim::slot_pass in csrc/sim/world.inc, Tile::SCAN_ONCE): the sensing candidates, the pre-checks of the
reveal / window phase and the fast-path test of the end-of-step GC come from one pass, taken again only behind a window expiry.  Every case
here steps the device next to the CPU oracle with no tolerance — every field and the observation rows after every step (Snapshot / compare
of test_gpu_parity) — and runs the same seeds once through the fused rollout.  The seeds were chosen with the oracle on the CPU; what makes a
case worth running (an expiry that frees a heading agent, a reveal with and without an expiry, a task retired and one created in one step,
the tile exactly full, runs of steps that change no list) is asserted from ORACLE state, so a case cannot go vacuous unnoticed."""
import numpy as np
import pytest

import orc
from cases import params_of
from test_gpu_parity import Snapshot, compare

pytestmark = pytest.mark.gpu

TILE16 = dict(tile_agents=16, tile_tasks=40, tile_threats=16)
# name -> (case, tile arguments, replan interval, seeds, steps, steps at which the fused rollout is stopped and compared)
RUNS = {
    # 16 x 40, hard windows: every seed has a window that runs out on a task a live agent is still flying to, by step 73 at the latest
    "hard_x2": ("WPS_hard_x2", {}, 20, (0, 1, 3, 5, 6, 7, 12, 15), 80, (36, 80)),
    # 24 x 48: the escort sync (creates and retires escort tasks, moves them) runs in front of the pass; reveal + expiry meet in step 32
    "escort24": ("WPS_escort24", {}, 12, (0, 1, 2, 3), 50, (32, 50)),
    # WIDE1000488 (tests/golden/wide_configs.json) on the 40-slot tile: these seeds fill it exactly (40 held task ids) and do not pass it
    # within 43 steps; seed 57 retires a task and creates one in a step that leaves it full
    "wide_full": ("WIDE1000488", TILE16, 20, (57, 47, 44), 43, (43,)),
}
SLOTS = {"hard_x2": 40, "escort24": 48, "wide_full": 40}


def _params(name):
    case, tiles = RUNS[name][:2]
    return params_of(case, **tiles)


def _env(name, n):
    from muavta_amd.batched import BatchedMultiUAVEnv
    return BatchedMultiUAVEnv(_params(name), n)


def _oracle_view(o):
    rows, _ = o.tasks()
    ag, _, q = o.agents()
    return rows, ag, q, o.list_sizes(), o.open_ids().copy()


def _classify(o, before, after, slots):
    """What the step between two oracle views did to the task lists (sets of tags)."""
    (rows0, ag0, q0, sz0, open0), (rows1, _, _, sz1, open1) = before, after
    tnow, n0 = o.dims()["time_steps"], len(rows0)
    st0, st1, dl = rows0[:, 0], rows1[:n0, 0], rows0[:, 7]
    retired = [k for k in range(1, n0) if st0[k] != 2 and st1[k] == 2]
    expired = [k for k in retired if dl[k] >= 0 and tnow > dl[k]]  # (a task concluded in the very step its window ran out counts too: rare, and the next tag does not)
    tags = set()
    for k in expired:  # ... freed by the expiry for certain: every live agent heading it was still under way (state 1), so nobody concluded it in this step
        heads = [a for a in range(o.A) if ag0[a, 2] != -1 and q0[a, 0] == k]
        if heads and all(ag0[a, 2] == 1 for a in heads):
            tags.add("expiry_frees_heading_agent")
    reveal = sz1["n_pending"] < sz0["n_pending"]  # (entries are only ever added or revealed: fewer than before means one came due)
    created = len(rows1) > n0
    if reveal and expired: tags.add("reveal_and_expiry")
    if reveal and not retired: tags.add("reveal_alone")
    if retired and created: tags.add("retire_and_create")
    if not retired and not created and np.array_equal(open0, open1): tags.add("quiet")
    if sz1["n_held"] == slots: tags.add("tile_full")  # (task ids a device slot is held for: not retired, or still queued by a live agent)
    if retired and created and sz1["n_held"] == slots: tags.add("retire_and_create_full")
    return tags


_DONE = {}


def _stepwise(name):
    """reset + steps x (allocate -> step) on the device (k_allocate, k_step) next to the oracle, compared after every step; per env the tags of
    every step.  Made once per run."""
    if name in _DONE:
        return _DONE[name]
    case, _, interval, seeds, steps, _ = RUNS[name]
    n = len(seeds)
    env = _env(name, n)
    oracles = [orc.OracleEnv(_params(name)) for _ in seeds]
    for o, s in zip(oracles, seeds):
        o.reset(s)
    env.reset(np.array(seeds, dtype=np.uint64))
    tags = [[] for _ in seeds]
    for t in range(steps):
        aa, ai = env.allocate(interval, True)
        views = []
        for i, o in enumerate(oracles):
            oa, oi = o.allocate(interval, 1)
            k = len(oa)
            assert np.array_equal(aa[i][:k], oa) and np.all(aa[i][k:] == -1) and np.array_equal(ai[i][:k], oi), f"{name} seed {seeds[i]} t={t}: plan"
            views.append(_oracle_view(o))
            o.step(oa, oi)
        env.step(aa, ai)
        snap = Snapshot(env)
        for i, o in enumerate(oracles):
            compare(snap, i, o, f"{name} seed {seeds[i]} t={t + 1}")
            tags[i].append(_classify(o, views[i], _oracle_view(o), SLOTS[name]))
    _DONE[name] = tags
    return tags


def _count(tags, tag):
    return [sum(tag in s for s in per_env) for per_env in tags]


def _fused(name):
    case, _, interval, seeds, _, stops = RUNS[name]
    n = len(seeds)
    for stop in stops:
        env = _env(name, n)
        env.rollout(np.array(seeds, dtype=np.uint64), stop, interval, True, True)
        snap = Snapshot(env)
        for i, s in enumerate(seeds):
            o = orc.OracleEnv(_params(name))
            assert o.rollout(s, stop, interval, 1) == stop
            compare(snap, i, o, f"{name} fused seed {s} after {stop} steps")


def test_window_expiry_frees_a_heading_agent_stepwise():
    """WPS_hard_x2, 16 x 40: in every env some step expires a window while a live agent heads that task — status, TF_REACHED and the queues
    change behind the pass, which is taken again there (blocking / idle / responding for step_serial_c, ret for the GC)."""
    per_env = _count(_stepwise("hard_x2"), "expiry_frees_heading_agent")
    assert min(per_env) >= 1, f"(env, step) pairs with such an expiry, per env: {per_env}"


def test_reveals_with_and_without_an_expiry_stepwise():
    """A step in which a reveal is due and a window expires (both halves of process_lists_coop, then the second pass), and steps in which a
    reveal is due and nothing retires (the results of the first pass are used as they are)."""
    tags = _stepwise("hard_x2")
    both, alone = sum(_count(tags, "reveal_and_expiry")), _count(tags, "reveal_alone")
    assert both >= 1 and min(alone) >= 1, f"reveal + expiry steps: {both}; reveal-only steps per env: {alone}"


def test_retire_and_create_in_one_step_and_quiet_steps_stepwise():
    """A task retired and one created in the same step (the end-of-step fast path must not be taken: the handed-over bits say so), and at
    least a quarter of all (env, step) pairs that change no task list (the fast path runs on the handed-over bits)."""
    tags = _stepwise("hard_x2")
    rc, quiet, total = sum(_count(tags, "retire_and_create")), sum(_count(tags, "quiet")), sum(len(t) for t in tags)
    assert rc >= 1 and 4 * quiet >= total, f"retire + create steps: {rc}; quiet (env, step) pairs: {quiet} of {total}"


def test_fused_rollout_of_the_same_seeds():
    """The same seeds through k_rollout, stopped behind the first expiries and at the end."""
    _fused("hard_x2")


def test_escort_sync_in_front_of_the_pass_stepwise_and_fused():
    """WPS_escort24 (24 x 48): escort tasks are created, moved and retired by the sync right in front of the pass; a reveal and an expiry
    that frees a heading agent meet in one step.  (The shipped library switches the pass on for the 16-agent tile only, MUAVTA_SCAN_ONCE=1:
    this case runs the three-walk step there and the one-pass step on a build with bit 2 of the knob set.)"""
    tags = _stepwise("escort24")
    assert min(_count(tags, "expiry_frees_heading_agent")) >= 1 and min(_count(tags, "reveal_and_expiry")) >= 1
    _fused("escort24")


def test_full_tile_stepwise_and_fused():
    """WIDE1000488 with all 40 slots of the tile held: every env reaches that, one retires and creates a task in a step that ends full (a
    slot recycled within the step sits at the end of t_order and at its old row of last_tasks_info: lists of equal length that differ)."""
    tags = _stepwise("wide_full")
    full, rc_full = _count(tags, "tile_full"), sum(_count(tags, "retire_and_create_full"))
    assert min(full) >= 1 and rc_full >= 1, f"steps that end with the tile full, per env: {full}; with a task retired and one created: {rc_full}"
    _fused("wide_full")
