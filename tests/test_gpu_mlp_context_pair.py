"""The learned MLP-ContextPair policy on the device (muavta_set_context_pair_policy + MUAVTA_ALLOC_MLP_PAIR, csrc/sim/policy.inc) against its
host twin (tests/policy_mlp_py.py: the arithmetic contract, bit for bit up to the logits), against the reference's recorded episodes
(tools/gen_golden_mlp_context_pair.py) and against itself along every path that carries the mode (fused rollout, stepwise allocate,
pair_scores -> allocate_scored, parts, lanes, policy swaps).  Tolerances: none on logits and on anything between device paths; scores
against the reference's float64 evaluation within 4 x D_ref of the trace, D_ref = the reference's own float32 deviation from that
evaluation, read from the fixture (never measured on the device)."""
import glob
import os

import numpy as np
import pytest

import policy_mlp_py as twin
from muavta_amd.native import MuavtaError
from test_gpu_mlp_pair import _env, compare_paths, full_state, stepwise

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TRACES = sorted(glob.glob(os.path.join(GOLDEN, "mlpctx_trace_*.npz")))
METRICS = sorted(glob.glob(os.path.join(GOLDEN, "mlpctx_metrics_*.npz")))
TILE_CASES = [("WPS_hard", 16), ("WPS_escort24", 24), ("WPS_burst64", 64)]
BOUND = 4.0  # x D_ref


def _weights(name):
    return twin.load_weights(twin.CONTEXT, name)


def _pair_weights(name):
    return twin.load_weights(twin.PAIR, name)


def _policy_env(case, n, wname, **kw):
    env = _env(case, n, **kw)
    w = _weights(wname)
    env.set_pair_policy(twin.as_state_dict(w))
    env.set_allocator("mlp_context_pair")
    return env, w


def _kind(w):
    return "pair_raw" if w["raw_features"] else "pair"


def check_against_twin(env, w, tag, seen):
    """logits of every env's current state, bit for bit; `seen` collects which kinds of state were met"""
    tok = env.tokens(_kind(w), 32, 16)
    ctx = env.context(_kind(w), 32)
    scores, logits = env.pair_scores(want_logits=True)
    ts, tl = twin.forward_batch(twin.CONTEXT, w, dict(tok, context=ctx))
    ev = tok["edge_valid"] != 0
    diff = logits.view(np.uint32) != tl.view(np.uint32)
    assert not diff.any(), f"{tag}: {int(diff.sum())} of {int(ev.sum())} logits differ from the host twin"
    assert not scores[~ev].any() and not logits[~ev].any(), f"{tag}: masked entries"
    # tanhf against numpy's float32 tanh: a few ulp of the score range
    assert np.abs(scores.astype(np.float64) - ts)[ev].max(initial=0.0) <= 4 * np.spacing(np.float32(w["score_clamp"])), tag
    per_env = ev.sum(axis=(1, 2))
    seen["second_pass"] |= bool((per_env > 64).any())
    seen["no_valid_pair"] |= bool((per_env == 0).any())
    seen["few_agents"] |= bool(((tok["agent_mask"] == 0).sum(axis=1) < 16).any())
    seen["no_open_task"] |= bool(((tok["task_mask"] == 0).sum(axis=1) == 0).any())
    return int(ev.sum())


# 1. logits, bit for bit
@pytest.mark.parametrize("wname", ["init2", "init2_raw", "il3"])
@pytest.mark.parametrize("case,tile", TILE_CASES)
def test_logits_equal_the_host_twin_bit_for_bit(case, tile, wname):
    """8 envs stepped through their episodes in the mode; the states checked on the way include envs with more than 64 valid pairs (a second
    pass over the list), with no valid pair, with fewer than 16 live agents (pad agent rows: the pool's divisor is not 16) and with no
    open task (t_pool = 0 / max(0, 1)) — which case brings which is asserted below, for every weight set, raw features included."""
    n = 8
    env, w = _policy_env(case, n, wname)
    assert env.A_tile == tile
    env.reset(np.arange(n, dtype=np.uint64) + 11)
    seen = dict(second_pass=False, no_valid_pair=False, few_agents=False, no_open_task=False)
    checked = 0
    for t in range(150):
        if t < 2 or t % 13 == 0:
            checked += check_against_twin(env, w, f"{case} {wname} t={t}", seen)
        env.allocate(15, True, fetch=False)
        env.step_staged()
    checked += check_against_twin(env, w, f"{case} {wname} end", seen)
    print(f"{case} {wname}: {checked} logits, states met {seen}")
    assert checked > 1000 and not env.get("ERROR").any()
    assert seen["no_valid_pair"]
    if tile == 64:
        assert seen["second_pass"]
    if tile == 16:
        assert seen["few_agents"]
    if tile != 24:  # (the escort case keeps escort tasks open to the end; the other two run out of open tasks: every task row a pad, t_pool = 0 / 1)
        assert seen["no_open_task"]


def test_states_without_an_open_task_and_with_few_agents():
    """The edge states of the pools, reached by stepping: WPS_hard episodes end with every task done (no open task: every task row a pad,
    t_pool = +0.0) and lose agents on the way (a_pool over fewer than 16 rows)."""
    n = 16
    env, w = _policy_env("WPS_hard", n, "init2")
    env.reset(np.arange(n, dtype=np.uint64) + 300)
    seen = dict(second_pass=False, no_valid_pair=False, few_agents=False, no_open_task=False)
    for t in range(150):
        env.allocate(15, True, fetch=False)
        env.step_staged()
        if t % 30 == 29:
            check_against_twin(env, w, f"t={t}", seen)
    tok = env.tokens("pair", 32, 16)
    print("states met", seen, "open tasks at the end", (tok["task_mask"] == 0).sum(axis=1))
    assert seen["few_agents"] and seen["no_valid_pair"] and seen["no_open_task"]


def test_tanhf_over_its_range():
    """Layer 3 of init2 scaled by 24 (logits to beyond +-4): logits still bit for bit against the host twin, scores against tanh of the SAME
    logit evaluated in float64, times score_clamp.  Bound: 4 spacings of score_clamp, as for MLP-Pair."""
    n = 16
    w = _weights("init2")
    w["w2"], w["b2"] = (w["w2"] * np.float32(24)).astype(np.float32), (w["b2"] * np.float32(24)).astype(np.float32)
    env = _env("WPS_hard_x2", n)
    env.set_pair_policy(twin.as_state_dict(w))
    env.set_allocator("mlp_pair")
    env.reset(np.arange(n, dtype=np.uint64) + 40)
    lo, hi, worst = 0.0, 0.0, 0.0
    for t in range(60):
        if t % 15 == 0:
            tok, ctx = env.tokens("pair", 32, 16), env.context("pair", 32)
            scores, logits = env.pair_scores(want_logits=True)
            _, tl = twin.forward_batch(twin.CONTEXT, w, dict(tok, context=ctx))
            ev = tok["edge_valid"] != 0
            assert np.array_equal(logits.view(np.uint32), tl.view(np.uint32))
            want = np.tanh(logits.astype(np.float64)) * np.float64(np.float32(w["score_clamp"]))
            worst = max(worst, float(np.abs(scores.astype(np.float64) - want)[ev].max()))
            lo, hi = min(lo, float(logits[ev].min())), max(hi, float(logits[ev].max()))
        env.allocate(15, True, fetch=False)
        env.step_staged()
    bound = 4 * float(np.spacing(np.float32(w["score_clamp"])))
    print(f"logits span {lo:.2f} .. {hi:.2f}; max |score - tanh64(logit) * clamp| {worst:.3e} (bound {bound:.3e})")
    assert lo < -3 and hi > 3, (lo, hi)
    assert worst <= bound


# 2. scores vs the reference, along the reference's trajectory
def replay(path):
    """env 0 follows the reference's episode exactly (allocate_scored fed the fixture's torch scores); at every plan the device's tokens and
    context must equal the fixture's and the device's scores are compared with the fixture's float64 evaluation."""
    g = np.load(path)
    case, wname, interval, seed = str(g["case"]), str(g["weights"]), int(g["interval"]), int(g["seed"])
    env, w = _policy_env(case, 1, wname)
    kind = _kind(w)
    env.reset(np.array([seed], dtype=np.uint64))
    worst, k = 0.0, 0
    for t in range(len(g["replanned"])):
        planned = bool(g["replanned"][t])
        sc = np.zeros((1, 16, 32), np.float32)
        if planned:
            assert t == int(g["step"][k])
            tok = env.tokens(kind, 32, 16)
            assert np.array_equal(tok["task_feats"][0], g["tf"][k]) and np.array_equal(tok["agent_feats"][0], g["af"][k]) and np.array_equal(tok["edge_valid"][0], g["ev"][k]) \
                and np.array_equal(tok["task_mask"][0], g["tmask"][k]) and np.array_equal(tok["agent_mask"][0], g["amask"][k]), f"{os.path.basename(path)} t={t}: tokens vs reference"
            assert np.array_equal(env.context(kind, 32)[0].view(np.uint32), g["ctx"][k].view(np.uint32)), f"t={t}: context vs reference"
            got = env.pair_scores()[0]
            ev = g["ev"][k] != 0
            assert not got[~ev].any()
            if ev.any():
                worst = max(worst, float(np.abs(got.astype(np.float64) - g["scores64"][k])[ev].max()))
            sc[0] = g["scores"][k]
        out = env.allocate_scored(kind, 32, 16, edge_scores=sc, gate="trainer", replan_interval=interval)
        assert bool(out["replanned"][0]) == planned, f"t={t}: gate"
        if planned:
            assert np.array_equal(out["selected"][0], g["selected"][k]), f"t={t}: selected mask vs reference"
            k += 1
        env.step_staged()
    assert k == len(g["step"]) and not env.get("ERROR").any()
    assert np.array_equal(env.metrics()[0], g["metrics"]) and int(env.get("SCALARS")[0, 23]) == int(g["n_replans"])
    return worst


@pytest.mark.parametrize("path", TRACES, ids=lambda p: os.path.basename(p)[:-4])
def test_scores_vs_reference_along_its_trajectory(path):
    D = float(np.load(path)["d_ref"])
    assert D > 0
    worst = replay(path)
    print(f"{os.path.basename(path)}: D_ref {D:.3e}, device max |score - scores64| {worst:.3e}, ratio {worst / D:.2f} (bound {BOUND})")
    assert worst <= BOUND * D


# 3. the chain, bit for bit
@pytest.mark.parametrize("case,tile,interval,use_vis,wname", [("WPS_hard", 16, 15, True, "init2"), ("WPS_escort24", 24, 20, False, "init2_raw"),
                                                              ("WPS_burst64", 64, 20, True, "il3")])
def test_fused_equals_stepwise_equals_scored_chain(case, tile, interval, use_vis, wname):
    """Every env of the batch is compared, none with a tolerance: every field of the state, the metrics and n_replans, fused == stepwise ==
    pair_scores -> allocate_scored.  An env whose episode ends before the last step is compared at the step it ended (the fused loop stops
    stepping it there, the stepwise loops keep stepping).  An env that outgrows the escort tile's pending-reveal list stops with ERROR set
    in every path alike and is excluded, as in the MLP-Pair test, which sees 24 of 384 such envs: at most that share (1 in 16) here."""
    import torch
    n, steps = 64, 150
    seeds = np.arange(n, dtype=np.uint64) + 100
    fused, w = _policy_env(case, n, wname)
    assert fused.A_tile == tile
    fused.rollout(seeds, steps, interval, use_vis, True)
    rm = fused.rollout_metrics()
    A = full_state(fused)
    assert np.array_equal(A["metrics"], rm)

    step, _ = _policy_env(case, n, wname)
    path_b = stepwise(step, seeds, steps, lambda e: e.allocate(interval, use_vis, fetch=False))
    chain, _ = _policy_env(case, n, wname)
    chain.set_allocator("hungarian")  # the scores come through the stand-alone kernel: no allocator mode involved
    sc = torch.empty((n, 16, 32), dtype=torch.float32, device=torch.device("cuda", chain.device_index))

    def plan_chain(e):
        e.pair_scores(out={"scores": sc})
        e.allocate_scored(_kind(w), 32, 16, edge_scores=sc, gate="trainer", replan_interval=interval, use_visibility=use_vis, edge_valid_only=True, out={})
    full, n_early = compare_paths(case, A, path_b, stepwise(chain, seeds, steps, plan_chain))
    compared = full + n_early
    print(f"{case} {wname} interval {interval} vis {use_vis}: {n} envs, {full} compared in full at step {steps}, {n_early} at their earlier end, "
          f"{n - compared} outgrew the tile")
    assert (n - compared) * 16 <= n, f"{n - compared} of {n} envs outgrew the tile"
    assert A["SCALARS"][:, 23].max() >= 5  # plans were made
    if tile != 24:
        assert not A["ERROR"].any() and compared == n


# 4. episodes vs the reference
def groups():
    out = {}
    for p in METRICS:
        g = np.load(p)
        out.setdefault((str(g["weights"]), int(g["interval"])), []).append(p)
    return sorted(out.items())


@pytest.mark.parametrize("key,paths", groups(), ids=lambda v: f"{v[0]}_i{v[1]}" if isinstance(v, tuple) else None)
def test_fused_episodes_vs_reference(key, paths):
    """Fused metrics and n_replans against the reference's float32 column.  A last-bit difference in a score can flip a near-tie, after
    which the episode diverges, so the cap follows the reference's own behaviour: with F_ref = the episodes whose float32 and float64
    columns differ, at most max(2, 2 x F_ref) of the 48 episodes recorded for init2 under the wps_eval loop may differ; the two
    8-episode groups get 2 x F_ref."""
    wname, interval = key
    E = F = 0
    differing = []
    for p in paths:
        g = np.load(p)
        case, n = str(g["case"]), g["metrics32"].shape[0]
        F += sum(not (np.array_equal(a, b) and ra == rb) for a, b, ra, rb in zip(g["metrics32"], g["metrics64"], g["n_replans32"], g["n_replans64"]))
        E += n
        env, _ = _policy_env(case, n, wname)
        env.rollout(np.arange(n, dtype=np.uint64), 150, interval, True, True)
        got, reps = env.rollout_metrics(), env.get("SCALARS")[:, 23].astype(np.int64)
        assert not env.get("ERROR").any()
        for s in range(n):
            if not (np.array_equal(got[s], g["metrics32"][s]) and reps[s] == g["n_replans32"][s]):
                differing.append((case, s))
    cap = max(2, 2 * F) if wname == "init2" else 2 * F
    print(f"{wname} interval {interval}: E = {E}, F_ref = {F}, device differs in {len(differing)} episodes {differing} (cap {cap})")
    assert len(differing) <= cap, differing


# 5. parts, lanes, swaps
def test_parts_two_lanes_and_a_late_second_lane():
    case, n = "WPS_attn", 64
    sets = [np.arange(k * 1000, k * 1000 + n, dtype=np.uint64) for k in range(2)]
    one, _ = _policy_env(case, n, "init2")
    one.set_lanes(1)
    want = []
    for sd in sets:
        one.rollout(sd, 150, 15, True, True)
        one.sync()
        want.append(one.rollout_metrics())
        assert not one.get("ERROR").any()
    assert not np.array_equal(want[0], want[1])
    # two seeded batches back to back on two lanes; the second lane is created AFTER the policy and the mode were set and gets its copy
    two, _ = _policy_env(case, n, "init2")
    two.set_lanes(2)
    for sd in sets:
        two.rollout(sd, 150, 15, True, True)
    assert np.array_equal(two.rollout_metrics(back=1), want[0]) and np.array_equal(two.rollout_metrics(), want[1])
    # a policy set while both lanes exist reaches both
    ref_il, _ = _policy_env(case, n, "il3")
    ref_il.rollout(sets[0], 150, 15, True, True)
    two.set_pair_policy(twin.as_state_dict(_weights("il3")))
    for sd in (sets[0], sets[0]):
        two.rollout(sd, 150, 15, True, True)
    assert np.array_equal(two.rollout_metrics(back=1), ref_il.rollout_metrics()) and np.array_equal(two.rollout_metrics(), ref_il.rollout_metrics())
    # sub-batches: fused per part, and stepwise per part
    parts, _ = _policy_env(case, n, "init2")
    parts.reset(sets[0])
    parts.set_parts(2)
    for p in range(2):
        parts.rollout_part(p, 150, 15, True, True)
    parts.sync()
    assert np.array_equal(parts.metrics(), want[0]) and not parts.get("ERROR").any()
    parts.reset(sets[1])
    for t in range(150):
        for p in range(2):
            parts.allocate_part(p, 15, True, fetch=False)
            parts.step_part(p, None, None)
    parts.sync()
    by_parts = parts.metrics()
    parts.set_parts(0)
    stepwise, _ = _policy_env(case, n, "init2")
    stepwise.reset(sets[1])
    for t in range(150):
        stepwise.allocate(15, True, fetch=False); stepwise.step_staged()
    assert np.array_equal(by_parts, stepwise.metrics())


def test_swapping_pair_context_pair_between_rollouts():
    """Either setter replaces a policy of the other kind: pair, context, pair between rollouts on one handle (two lanes), each result equal
    to a fresh handle's."""
    case, n = "WPS_hard_x2", 32
    seeds = np.arange(n, dtype=np.uint64) + 7
    wp, wc = _pair_weights("init2"), _weights("init2")

    def fresh(sd):
        e = _env(case, n)
        e.set_pair_policy(sd)
        e.set_allocator("mlp_pair")
        e.rollout(seeds, 150, 15, True, True)
        return e.rollout_metrics(), e.pair_scores()
    want_p, sc_p = fresh(twin.as_state_dict(wp))
    want_c, sc_c = fresh(twin.as_state_dict(wc))
    assert not np.array_equal(want_p, want_c) and not np.array_equal(sc_p, sc_c)
    env = _env(case, n)
    env.set_lanes(2)
    env.set_pair_policy(twin.as_state_dict(wp))
    env.set_allocator("mlp_pair")
    with pytest.raises(MuavtaError, match="MLP-ContextPair"):
        env.set_allocator("mlp_context_pair")
    for sd, want, sc in ((twin.as_state_dict(wp), want_p, sc_p), (twin.as_state_dict(wc), want_c, sc_c), (twin.as_state_dict(wp), want_p, sc_p)):
        env.set_pair_policy(sd)
        env.rollout(seeds, 150, 15, True, True)
        assert np.array_equal(env.rollout_metrics(), want)
        assert np.array_equal(env.pair_scores(), sc)
    assert not env.get("ERROR").any()


# 6. refusals
def test_refusals_leave_the_handle_usable():
    import ctypes as C
    import torch
    from muavta_amd import native
    case, n = "WPS_hard", 4
    env = _env(case, n)
    seeds = np.arange(n, dtype=np.uint64)
    with pytest.raises(MuavtaError, match="MLP-ContextPair"):
        env.set_allocator("mlp_context_pair")
    env.reset(seeds)
    w = _weights("init2")
    z = np.zeros(192 * 192, np.float32)
    for spec, word in ((native.MuavtaContextPairMlp(0, 128, 0.35, *([z.ctypes.data] * 6)), b"hidden"), (native.MuavtaContextPairMlp(2, 192, 0.35, *([z.ctypes.data] * 6)), b"raw_features"),
                       (native.MuavtaContextPairMlp(0, 192, 0.35, z.ctypes.data, None, *([z.ctypes.data] * 4)), b"non-null")):
        assert env.L.muavta_set_context_pair_policy(env.h, C.byref(spec)) == -1 and word in env.L.muavta_last_error(env.h)
    assert env.L.muavta_set_allocator(env.h, 7) == -1 and env.L.muavta_set_allocator(env.h, 6) == -5  # MUAVTA_E_ARG: unknown mode; MUAVTA_E_STATE: no policy yet
    env.rollout(seeds, 150, 20, True, True)   # still the Hungarian handle it was
    fresh = _env(case, n)
    fresh.rollout(seeds, 150, 20, True, True)
    assert np.array_equal(env.rollout_metrics(), fresh.rollout_metrics())
    env.set_pair_policy(twin.as_state_dict(w))
    env.set_allocator("mlp_context_pair")
    with pytest.raises(MuavtaError, match="selected"):
        env.set_pair_policy(None)
    assert env.L.muavta_set_context_pair_policy(env.h, None) == -5 and b"selected" in env.L.muavta_last_error(env.h)
    dev = torch.device("cuda", env.device_index)
    rings = {k: torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device=dev) for k, (shape, dt) in env.obs_ring_shapes(20).items()}
    with pytest.raises(MuavtaError, match="MLP-Pair"):
        env.rollout_record(seeds, 20, 15, True, obs_rings=rings)
    env.rollout(seeds, 150, 15, True, True)
    ref, _ = _policy_env(case, n, "init2")
    ref.rollout(seeds, 150, 15, True, True)
    assert np.array_equal(env.rollout_metrics(), ref.rollout_metrics())
    env.set_allocator("hungarian")
    assert env.L.muavta_set_context_pair_policy(env.h, None) == 0  # NULL clears, through either setter
    env._pair_policy = None
    with pytest.raises(MuavtaError, match="set_pair_policy"):
        env.set_allocator("mlp_pair")
    env.rollout(seeds, 150, 20, True, True)
    assert np.array_equal(env.rollout_metrics(), fresh.rollout_metrics())
