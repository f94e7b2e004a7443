"""CPU side of the MT19937 block-boundary tests: the oracle's word counter against real CPython, the fact that no 150-step registry
episode draws a whole block from one stream, and a guard on every (configuration, seed) test_gpu_rng_blocks.py uses — if a model
change moves the draws, this file fails instead of the GPU tests silently losing their coverage."""
import random

import numpy as np
import pytest

import orc
import rng_blocks as rb
from muavta_amd.params import METRIC_KEYS, params_for_case

N_ARRIVALS = METRIC_KEYS.index("n_arrivals")


def test_stream_seeds_and_raw_blocks_helpers_against_cpython():
    """mt_blocks() returns the raw state CPython tempers its outputs from: tempering block b by hand gives getrandbits(32) number
    624 * b .. 624 * b + 623 of a fresh generator."""
    for seed in (0, 12345, 2 ** 32, 2 ** 63 - 1):
        blocks = rb.mt_blocks(seed, 3)
        y = blocks.astype(np.uint64).ravel()
        y ^= y >> np.uint64(11)
        y ^= (y << np.uint64(7)) & np.uint64(0x9D2C5680)
        y ^= (y << np.uint64(15)) & np.uint64(0xEFC60000)
        y ^= y >> np.uint64(18)
        r = random.Random(seed)
        assert [int(v) for v in y] == [r.getrandbits(32) for _ in range(3 * 624)]


@pytest.mark.parametrize("name,seed", [("hard700", 0), ("hard700", 2 ** 40 + 12345), ("escort700", 3), ("burst64_random_init", 0)])
def test_oracle_streams_against_cpython_past_two_blocks(name, seed):
    """The four stream seeds of reset(seed) are Random(seed) and three randint(0, 2**63 - 1) from it; the oracle's generator seeded with
    each gives CPython's words over two block ends (1300 words), and its count of them only moves forward: it is the same after
    an episode run in one go and in pieces that stop around every crossing."""
    L, C = orc.lib(), orc.C
    for st, ss in enumerate(rb.stream_seeds(seed)):
        r = random.Random(ss)
        g = C.c_void_p(L.orc_rng_new(C.c_uint64(ss)))
        try:
            for k in range(650):  # random() takes two words
                assert L.orc_rng_random(g) == r.random(), f"stream {rb.STREAMS[st]} words {2 * k}, {2 * k + 1}"
        finally:
            L.orc_rng_free(g)
    words, _, _ = rb.trace(name, seed)
    assert len(words) == rb.horizon(name) + 1
    assert words[-1].max() > (1248 if name != "burst64_random_init" else 624)
    assert np.all(np.diff(words, axis=0) >= 0)
    stops = sorted({0, len(words) - 1} | {t + d for (t, _, _, _) in rb.crossings(words) for d in (0, 1, 2)})
    o = orc.OracleEnv(rb.params(name))
    o.reset(seed)
    done = 0
    for stop in stops:
        assert o.rollout(0, stop - done, rb.interval(name), 1, do_reset=0) == stop - done
        done = stop
        assert o.rng_words() == words[stop].tolist()
    o.reset(seed)  # seed() zeroes the count
    assert o.rng_words() == words[0].tolist()


def test_counter_follows_the_models_draws_step_by_step():
    """The count and the values together: replay the tgt stream of a hard700 episode with random.Random.  _maybe_arrival draws
    random() every step (2 words) and more when a task arrives, so the replayed generator, advanced by exactly the counted words,
    must give the arrival decision the oracle took (n_arrivals grows exactly when random() < arrival_rate and the list has room)."""
    name, seed = "hard700", 2
    p = rb.params(name)
    o = orc.OracleEnv(p)
    o.reset(seed)
    r = random.Random(rb.stream_seeds(seed)[rb.TGT])
    for _ in range(o.rng_words()[rb.TGT]):
        r.getrandbits(32)
    checked = arrived = 0
    for t in range(rb.horizon(name)):
        before, ids_before = o.rng_words()[rb.TGT], o.dims()["n_task_ids"]
        oa, oi = o.allocate(rb.interval(name), 1)
        o.step(oa, oi)
        drawn = o.rng_words()[rb.TGT] - before
        if drawn:
            arrives = r.random() < p.arrival_rate and ids_before - 1 < p.max_tasks - 1  # (a full task list turns the arrival away)
            assert (drawn > 2) == arrives, f"t={t}: {drawn} words drawn"
            assert o.metrics()[N_ARRIVALS] == arrived + int(arrives), f"t={t}"
            arrived += int(arrives)
            for _ in range(drawn - 2):
                r.getrandbits(32)
            checked += 1
    assert o.rng_words()[rb.TGT] > 1248 and checked > 600 and arrived >= 10


@pytest.mark.parametrize("name,seed", sorted(rb.CROSSINGS, key=str), ids=lambda v: str(v))
def test_guard_crossings_the_gpu_tests_rely_on(name, seed):
    """Which stream passes word 624, at which step, from which offset, drawing how many words — and the episode reaches its horizon with
    an open list the device tile can hold."""
    words, open_max, o = rb.trace(name, seed)
    assert len(words) == rb.horizon(name) + 1 and o.dims()["truncated"]
    assert rb.crossings(words)[:len(rb.CROSSINGS[(name, seed)])] == rb.CROSSINGS[(name, seed)]
    if name != "burst64_random_init":
        assert rb.crossings(words) == rb.CROSSINGS[(name, seed)]
        assert words[-1, rb.TGT] > 1248 + 100  # draws follow the second flip of the marker
    assert open_max <= rb.OPEN_CAP[name]


@pytest.mark.parametrize("key", sorted(rb.RESET_WORDS, key=str), ids=lambda v: str(v))
def test_guard_resets_that_cross(key):
    name, seed = key
    o = orc.OracleEnv(rb.params(name))
    o.reset(seed)
    got = o.rng_words()
    for st, want in enumerate(rb.RESET_WORDS[key]):
        assert want is None or got[st] == want, f"{rb.STREAMS[st]}: {got[st]} words drawn by reset"
    assert got[rb.AGENT] >= 620 and got[rb.AGENT] > 160  # beyond the device's 160-word reset window; seeds 1, 2 (and tgt of seed 0) past the block end
    assert max(got) < 1248


def test_guard_inputs_of_the_other_gpu_tests():
    """The windows, seed lists and stop steps test_gpu_rng_blocks.py takes from rng_blocks.py."""
    g = rb
    for name, seeds, which in g.WINDOWS:  # (a): the compared window holds the crossing of every seed that has one there, and stays <= 16 steps
        first, last = g.window_of(name, seeds, which)
        assert last - first <= 16
        for s in seeds:
            if (name, s) in rb.CROSSINGS and len(rb.CROSSINGS[(name, s)]) > which:
                assert first + 3 <= rb.CROSSINGS[(name, s)][which][0] <= last - 5
    in_reset = 0
    for name in rb.CONFIGS:  # (b): every one of the 64 seeds passes a block end (on the 700-step configurations twice, in steps), never
        assert len(rb.FUSED_SEEDS[name]) == 64  # draws more than the two blocks a device tape holds, and no random_position() gives up
        for s in rb.FUSED_SEEDS[name]:
            words, _, o = rb.trace(name, s)
            assert len(words) == rb.horizon(name) + 1
            assert words[-1].max() >= 624, f"{name} seed {s}"
            assert rb.cursor_peak(words) <= 1248 and np.diff(words, axis=0).max() < 400, f"{name} seed {s}"
            assert not np.isnan(o.tasks()[0][:, 1:3]).any(), f"{name} seed {s}"
            if name != "burst64_random_init":
                assert len(rb.crossings(words)) == 2 and words[-1, rb.TGT] > 1248, f"{name} seed {s}"
            else:  # the agent stream of every seed passes word 624 within the episode, for more than half of them inside the reset
                assert words[-1, rb.AGENT] >= 624, f"{name} seed {s}"
                in_reset += int(words[0, rb.AGENT] >= 624)
    assert in_reset > 32
    for s in rb.BURST64_REJECTED:  # (why they are left out: the reset alone draws more than two blocks from the tgt stream)
        assert rb.trace("burst64_random_init", s, 0)[0][0, rb.TGT] > 1248
    words = rb.trace("burst64_random_init", 0, 3)[0]  # (c) / (d): the first step boundary finds a consumed block
    assert words[0, rb.AGENT] == 620 and words[0, rb.TGT] == 660 and words[1, rb.AGENT] < 624
    for s in range(8):
        assert max(rb.trace("burst64_random_init", s, 0)[0][0]) < 1248
    assert sum(rb.trace("burst64_random_init", s, 0)[0][0, rb.AGENT] >= 624 for s in range(8)) >= 5
    # (d): the stops end just after seed 0's crossings (regeneration due / done), and by 245 / 557 every seed has regenerated once / twice
    for s in g.TAPE_SEEDS:
        words, open_max, _ = rb.trace("hard700", s)
        c = rb.crossings(words)
        assert [x[1] for x in c] == ["tgt", "tgt"] and 230 <= c[0][0] <= 243 and 542 <= c[1][0] <= 555 and open_max <= 30, f"seed {s}: {c}"
        assert [int(words[stop - 1, rb.TGT]) // 624 for stop in (245, 557)] == [1, 2]
    w0 = rb.trace("hard700", 0)[0]
    assert [int(w0[stop, rb.TGT]) // 624 for stop in g.TAPE_STOPS] == [1, 1, 1, 2, 2, 2]          # the oracle's block
    assert [int(w0[stop - 1, rb.TGT]) // 624 for stop in g.TAPE_STOPS] == [0, 1, 1, 1, 2, 2]      # blocks the device has regenerated
    # (e): at t = 400 the tgt stream of seeds 0..7 is in block 1; (f): seeds 0..31 cross inside the single-step / three-step launches
    for s in range(32):
        words = rb.trace("hard700", s)[0]
        c = rb.crossings(words)
        assert words[400, rb.TGT] // 624 == 1 and words[399, rb.TGT] // 624 == 1
        if s < 16:
            assert 228 <= c[0][0] <= 242 and 540 <= c[1][0] <= 556, f"seed {s}: {c}"
        if s < 4:  # step_run: one launch holds the crossing step and the step after it (whose start regenerates the block), both times
            launches = rb.step_run_launches("hard700", s)
            for tc, _, _, _ in c:
                hit = [(t0, k) for t0, k in launches if t0 <= tc and t0 + k >= tc + 2]
                assert len(hit) == 1 and (200 <= hit[0][0] <= 260 or 520 <= hit[0][0] <= 580), f"seed {s}: {hit}"


def test_no_150_step_registry_episode_reaches_a_block_end():
    """WPS_burst64, the busiest registry case, seeds 1000..1063 at the 150 steps every other test runs: no stream draws 624 words.
    This is why the long-horizon configurations of rng_blocks.CONFIGS exist: without them nothing on the device ever regenerates a
    block, reads the other half of a tape or flips a block marker."""
    o = orc.OracleEnv(params_for_case("WPS_burst64"))
    top = np.zeros(4, dtype=np.int64)
    for seed in range(1000, 1064):
        o.rollout(seed, 150, 20, 1)
        top = np.maximum(top, o.rng_words())
    assert top.max() < 624, top
    assert top[rb.TGT] > 300  # (the counter counts: about 2 words per step and more per arrival)
