"""The learned MLP-Coalition policy on the device (muavta_set_pair_policy with raw_features = MUAVTA_TOK_ESCORT + MUAVTA_ALLOC_MLP_PAIR,
csrc/sim/policy.inc) against its host twin (tests/policy_mlp_py.py: the arithmetic contract, bit for bit up to the logits), against the
reference's recorded episodes (tools/gen_golden_mlp_coalition.py) and against itself along every path that carries the mode (fused rollout,
stepwise allocate, tokens -> pair_scores -> allocate_scored, lanes, policy swaps).  Tolerances: none on logits and on anything between device
paths; a score against sigmoid of its own logit in float64 within 4 x 2^-24 (division, expf and the add: about 1 ulp each on values <= 1 —
the project's "4 spacings" rule); scores against the reference's float64 evaluation within 4 x D_ref of the trace, D_ref = the
reference's own float32 deviation from that evaluation, read from the fixture (never measured on the device)."""
import glob
import os

import numpy as np
import pytest

import policy_mlp_py as twin
from muavta_amd.native import MuavtaError
from test_gpu_mlp_pair import _env, compare_paths, full_state, stepwise

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TRACES = sorted(glob.glob(os.path.join(GOLDEN, "mlpcoal_trace_*.npz")))
METRICS = sorted(glob.glob(os.path.join(GOLDEN, "mlpcoal_metrics_*.npz")))
TILE_CASES = [("WPS_hard", 16), ("WPS_escort24", 24), ("WPS_burst64", 64)]
BOUND = 4.0  # x D_ref
INTERVAL = 12
SCORE_BOUND = 4 * 2.0 ** -24


def _weights(name):
    return twin.load_weights(twin.COALITION, name)


def _policy_env(case, n, wname, **kw):
    env = _env(case, n, **kw)
    w = _weights(wname)
    env.set_pair_policy(twin.as_state_dict(w))
    env.set_allocator("mlp_coalition")
    return env, w


def check_against_twin(env, w, tag, seen):
    """logits of every env's current state, bit for bit; scores by the formula; `seen` collects which kinds of state were met"""
    tok = env.tokens("escort", 48, 16)
    scores, logits = env.pair_scores(want_logits=True)
    assert scores.shape == (env.n_envs, 16, 48)
    ts, tl = twin.forward_batch(twin.COALITION, w, tok)
    ev = tok["edge_valid"] != 0
    ok = ev & (tok["agent_mask"] == 0)[:, :, None] & (tok["task_mask"] == 0)[:, None, :]
    assert np.array_equal(ok, ev), f"{tag}: edge_valid set on a pad pair"
    diff = logits.view(np.uint32) != tl.view(np.uint32)
    assert not diff.any(), f"{tag}: {int(diff.sum())} of {int(ev.sum())} logits differ from the host twin"
    assert not scores[~ev].any() and not logits[~ev].any(), f"{tag}: masked entries"
    worst = float(np.abs(scores.astype(np.float64) - twin.sigmoid64(logits))[ev].max(initial=0.0))
    assert worst <= SCORE_BOUND, f"{tag}: |score - sigmoid64(clip(logit))| = {worst:.3e}"
    # the clip: beyond +-20 the score is sigmoid at +-20 itself.  sigmoid(20) = 1 - 2.1e-9 is 1.0f in float32 whatever expf's last bit;
    # sigmoid(-20) = 2.06e-9 goes through expf, one add and one division: within 4 spacings of its float32 value, and one value for every such pair
    hi, lo = ev & (logits > 20), ev & (logits < -20)
    assert np.all(scores[hi] == np.float32(1.0))
    s_lo = np.float32(twin.sigmoid64(-20.0))
    assert np.abs(scores[lo].astype(np.float64) - float(s_lo)).max(initial=0.0) <= 4 * float(np.spacing(s_lo)) and len(np.unique(scores[lo])) <= 1
    per_env = ev.sum(axis=(1, 2))
    seen["second_pass"] |= bool((per_env > 64).any())
    seen["over_384"] |= bool((per_env > 384).any())
    seen["no_valid_pair"] |= bool((per_env == 0).any())
    seen["few_agents"] |= bool(((tok["agent_mask"] == 0).sum(axis=1) < 16).any())
    seen["past_column_32"] |= bool(((tok["task_mask"] == 0).sum(axis=1) > 32).any())
    seen["clip_hi"] |= bool(hi.any())
    seen["clip_lo"] |= bool(lo.any())
    seen["max_pairs"] = max(seen.get("max_pairs", 0), int(per_env.max()))
    return int(ev.sum())


def _seen():
    return dict(second_pass=False, over_384=False, no_valid_pair=False, few_agents=False, past_column_32=False, clip_hi=False, clip_lo=False)


# 1. logits, bit for bit
@pytest.mark.parametrize("wname", ["init2", "ac3", "wide"])
@pytest.mark.parametrize("case,tile", TILE_CASES)
def test_logits_equal_the_host_twin_bit_for_bit(case, tile, wname):
    """8 envs per tile, the states after 0, 7 and 40 steps in the mode (WPS_hard: also the end of the episode), every weight set.  Which case
    brings which kind of state is asserted below: WPS_hard (16 x 40) envs with more than 64 valid pairs (a second pass over the list), with
    fewer than 16 live agents and, at the end, with no valid pair; WPS_escort24 a second pass; WPS_burst64 (64 x 128) envs whose task rows
    fill past column 32 and envs with more than 384 valid pairs — all 768 cells, twelve passes.  With the wide set the states of every tile reach both
    clip sides (t = 40 of the reference's own WPS_escort24 episode has 21 pairs above +20 and 6 below -20)."""
    n = 8
    seen = _seen()
    checked = 0
    env, w = _policy_env(case, n, wname)
    assert env.A_tile == tile
    env.reset(np.arange(n, dtype=np.uint64) + 11)
    last = 150 if tile == 16 else 40
    for t in range(last + 1):
        if t in (0, 7, 40, 150):
            checked += check_against_twin(env, w, f"{case} {wname} t={t}", seen)
        if t < last:
            env.allocate(INTERVAL, True, fetch=False)
            env.step_staged()
    print(f"{case} {wname}: {checked} logits, states met {seen}")
    assert checked > 1000 and not env.get("ERROR").any()
    if tile == 16:
        assert seen["second_pass"] and seen["few_agents"] and seen["no_valid_pair"]
    if tile == 24:
        assert seen["second_pass"]
    if tile == 64:
        assert seen["past_column_32"] and seen["over_384"] and seen["max_pairs"] == 768
    if wname == "wide":  # (on every tile: the clip assertions of check_against_twin had pairs to look at)
        assert seen["clip_hi"] and seen["clip_lo"]


# 2. scores vs the reference, along the reference's trajectory
def replay(path):
    """env 0 follows the reference's episode exactly (allocate_scored fed the fixture's torch scores); at every plan the device's tokens must
    equal the fixture's and the device's scores are compared with the fixture's float64 evaluation."""
    g = np.load(path)
    case, wname, interval, seed = str(g["case"]), str(g["weights"]), int(g["interval"]), int(g["seed"])
    env, w = _policy_env(case, 1, wname)
    env.reset(np.array([seed], dtype=np.uint64))
    worst, k = 0.0, 0
    for t in range(len(g["replanned"])):
        planned = bool(g["replanned"][t])
        sc = np.zeros((1, 16, 48), np.float32)
        if planned:
            assert t == int(g["step"][k])
            tok = env.tokens("escort", 48, 16)
            assert np.array_equal(tok["task_feats"][0], g["tf"][k]) and np.array_equal(tok["agent_feats"][0], g["af"][k]) and np.array_equal(tok["edge_valid"][0], g["ev"][k]) \
                and np.array_equal(tok["task_mask"][0], g["tmask"][k]) and np.array_equal(tok["agent_mask"][0], g["amask"][k]), f"{os.path.basename(path)} t={t}: tokens vs reference"
            got = env.pair_scores()[0]
            ev = g["ev"][k] != 0
            assert not got[~ev].any()
            if ev.any():
                worst = max(worst, float(np.abs(got.astype(np.float64) - g["scores64"][k])[ev].max()))
            sc[0] = g["scores"][k]
        out = env.allocate_scored("escort", 48, 16, edge_scores=sc, gate="escort", replan_interval=interval, edge_valid_only=False, commit=True)
        assert bool(out["replanned"][0]) == planned, f"t={t}: gate"
        if planned:
            assert np.array_equal(out["selected"][0], g["selected"][k]), f"t={t}: selected mask vs reference"
            assert np.array_equal(env.get("AGENT_MISC")[0, :env.n_agents, 4], g["commit_until"][k]), f"t={t}: commit locks vs reference"
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
@pytest.mark.parametrize("case,tile", [("WPS_hard", 16), ("WPS_escort", 24), ("WPS_burst64", 64)])
def test_fused_equals_stepwise_equals_scored_chain(case, tile):
    """16 envs x 150 steps, interval 12, none with a tolerance (the 24 x 48 tile with WPS_escort: under this policy most WPS_escort24 envs
    outgrow that tile's 88 pending reveals — 9 of these 16 seeds — in every path alike, which test_fused_episodes_vs_reference escalates): every field of the state (commit_until in AGENT_MISC, n_replans in SCALARS)
    and the metrics, fused == stepwise == tokens("escort") -> pair_scores -> allocate_scored(kind="escort", max_tasks=48, gate="escort",
    commit=True, edge_valid_only=False) -> step_staged.  An env whose episode ends before the last step is compared at the step it ended.
    Envs that flag a capacity error in every path alike are excluded; at least 12 of 16 must remain."""
    import torch
    n, steps = 16, 150
    seeds = np.arange(n, dtype=np.uint64) + 100
    fused, w = _policy_env(case, n, "init2")
    assert fused.A_tile == tile
    fused.rollout(seeds, steps, INTERVAL, True, True)
    rm = fused.rollout_metrics()
    A = full_state(fused)
    assert np.array_equal(A["metrics"], rm)

    step, _ = _policy_env(case, n, "init2")
    path_b = stepwise(step, seeds, steps, lambda e: e.allocate(INTERVAL, True, fetch=False))
    chain, _ = _policy_env(case, n, "init2")
    chain.set_allocator("hungarian")  # the scores come through the stand-alone kernel: no allocator mode involved
    sc = torch.empty((n, 16, 48), dtype=torch.float32, device=torch.device("cuda", chain.device_index))

    def plan_chain(e):
        e.pair_scores(out={"scores": sc})
        e.allocate_scored("escort", 48, 16, edge_scores=sc, gate="escort", replan_interval=INTERVAL, use_visibility=True, edge_valid_only=False, commit=True, out={})
    full, n_early = compare_paths(case, A, path_b, stepwise(chain, seeds, steps, plan_chain))
    compared = full + n_early
    print(f"{case} interval {INTERVAL}: {n} envs, {full} compared in full at step {steps}, {n_early} at their earlier end, {n - compared} outgrew the tile; "
          f"mean n_replans {A['SCALARS'][:, 23].mean():.1f}")
    assert compared >= 12, f"only {compared} of {n} envs could be compared"
    assert A["SCALARS"][:, 23].max() >= 5  # plans were made


# 4. episodes vs the reference
def groups():
    out = {}
    for p in METRICS:
        out.setdefault(str(np.load(p)["weights"]), []).append(p)
    return sorted(out.items())


@pytest.mark.parametrize("wname,paths", groups(), ids=lambda v: v if isinstance(v, str) else None)
def test_fused_episodes_vs_reference(wname, paths):
    """Fused metrics and n_replans against the reference's float32 column, with rollout(escalate=True): the reference's lists are unbounded,
    and under an untrained net most WPS_escort24 envs outgrow the 24 x 48 tile's 88 pending reveals (ERROR 4); those are re-run from their
    seeds on the 64 x 128 tile, same policy, same mode, and every one of the 48 + 8 episodes is compared.  A last-bit difference in a score can flip a near-tie, after
    which the episode diverges, so the cap follows the reference's own behaviour: with F_ref = the episodes whose float32 and float64
    columns differ, at most max(2, 2 x F_ref) of the 48 episodes recorded for init2 may differ; the ac3 group gets 2 x F_ref of its own file."""
    E = F = 0
    differing = []
    for p in paths:
        g = np.load(p)
        case, n = str(g["case"]), g["metrics32"].shape[0]
        F += sum(not (np.array_equal(a, b) and ra == rb) for a, b, ra, rb in zip(g["metrics32"], g["metrics64"], g["n_replans32"], g["n_replans64"]))
        E += n
        env, _ = _policy_env(case, n, wname)
        env.rollout(np.arange(n, dtype=np.uint64), 150, int(g["interval"]), True, True, escalate=True)
        got, reps = env.rollout_metrics(), env.get("SCALARS")[:, 23].astype(np.int64)
        for i, (h, row) in env.escalated.items():   # (an env no tile holds raises in rollout)
            reps[i] = int(h.get("SCALARS")[row, 23])
        print(f"{case}: {len(env.escalated)} of {n} envs re-run on the larger tile")
        for s in range(n):
            if not (np.array_equal(got[s], g["metrics32"][s]) and reps[s] == g["n_replans32"][s]):
                differing.append((case, s))
    cap = max(2, 2 * F) if wname == "init2" else 2 * F
    print(f"{wname}: E = {E}, F_ref = {F}, device differs in {len(differing)} episodes {differing} (cap {cap})")
    assert len(differing) <= cap, differing


# 5. lanes, swaps
def test_two_lanes_and_a_late_second_lane():
    case, n = "WPS_escort", 16
    sets = [np.arange(k * 1000, k * 1000 + n, dtype=np.uint64) for k in range(2)]
    one, _ = _policy_env(case, n, "init2")
    one.set_lanes(1)
    want = []
    for sd in sets:
        one.rollout(sd, 150, INTERVAL, True, True)
        one.sync()
        want.append(one.rollout_metrics())
        assert not one.get("ERROR").any()
    assert not np.array_equal(want[0], want[1])
    # two seeded batches back to back on two lanes; the second lane is created AFTER the policy and the mode were set and gets its copy
    two, _ = _policy_env(case, n, "init2")
    two.set_lanes(2)
    for sd in sets:
        two.rollout(sd, 150, INTERVAL, True, True)
    assert np.array_equal(two.rollout_metrics(back=1), want[0]) and np.array_equal(two.rollout_metrics(), want[1])
    # a policy set while both lanes exist reaches both
    ref_ac, _ = _policy_env(case, n, "ac3")
    ref_ac.rollout(sets[0], 150, INTERVAL, True, True)
    two.set_pair_policy(twin.as_state_dict(_weights("ac3")))
    for sd in (sets[0], sets[0]):
        two.rollout(sd, 150, INTERVAL, True, True)
    assert np.array_equal(two.rollout_metrics(back=1), ref_ac.rollout_metrics()) and np.array_equal(two.rollout_metrics(), ref_ac.rollout_metrics())


def test_swapping_pair_coalition_context_coalition_between_rollouts():
    """Either setter replaces a policy of another kind: pair, coalition, context, coalition between rollouts on one handle (two lanes), each
    result equal to a fresh handle's — the coalition kind's scratch block is created on the way and survives the other kinds."""
    case, n = "WPS_escort", 16
    seeds = np.arange(n, dtype=np.uint64) + 7
    sd_p = twin.as_state_dict(twin.load_weights(twin.PAIR, "init2"))
    sd_x = twin.as_state_dict(twin.load_weights(twin.CONTEXT, "init2"))
    sd_c = twin.as_state_dict(_weights("init2"))

    def fresh(sd, interval):
        e = _env(case, n)
        e.set_pair_policy(sd)
        e.set_allocator("mlp_pair")
        e.rollout(seeds, 150, interval, True, True)
        return e.rollout_metrics(), e.pair_scores()
    want_p, sc_p = fresh(sd_p, 15)
    want_x, sc_x = fresh(sd_x, 15)
    want_c, sc_c = fresh(sd_c, INTERVAL)
    assert sc_c.shape == (n, 16, 48) and sc_p.shape == (n, 16, 32) and not np.array_equal(want_p, want_c) and not np.array_equal(want_x, want_c)
    env = _env(case, n)
    env.set_lanes(2)
    env.set_pair_policy(sd_p)
    env.set_allocator("mlp_pair")
    with pytest.raises(MuavtaError, match="MLP-Coalition"):
        env.set_allocator("mlp_coalition")
    for sd, interval, want, sc in ((sd_p, 15, want_p, sc_p), (sd_c, INTERVAL, want_c, sc_c), (sd_x, 15, want_x, sc_x), (sd_c, INTERVAL, want_c, sc_c)):
        env.set_pair_policy(sd)
        env.rollout(seeds, 150, interval, True, True)
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
    with pytest.raises(MuavtaError, match="MLP-Coalition"):
        env.set_allocator("mlp_coalition")
    env.reset(seeds)
    z = np.zeros(256 * 256, np.float32)
    for spec, word in ((native.MuavtaPairMlp(2, 128, 0.35, *([z.ctypes.data] * 6)), b"hidden"), (native.MuavtaPairMlp(0, 256, 0.35, *([z.ctypes.data] * 6)), b"hidden"),
                       (native.MuavtaPairMlp(3, 256, 0.35, *([z.ctypes.data] * 6)), b"raw_features"),
                       (native.MuavtaPairMlp(2, 256, 0.35, z.ctypes.data, None, *([z.ctypes.data] * 4)), b"non-null")):
        assert env.L.muavta_set_pair_policy(env.h, C.byref(spec)) == -1 and word in env.L.muavta_last_error(env.h)
    spec = native.MuavtaContextPairMlp(2, 192, 0.35, *([z.ctypes.data] * 6))   # kind 2 through the other setter
    assert env.L.muavta_set_context_pair_policy(env.h, C.byref(spec)) == -1 and b"raw_features" in env.L.muavta_last_error(env.h)
    assert env.L.muavta_set_allocator(env.h, 7) == -1 and env.L.muavta_set_allocator(env.h, 6) == -5  # MUAVTA_E_ARG: unknown mode; MUAVTA_E_STATE: no policy yet
    env.rollout(seeds, 150, 20, True, True)   # still the Hungarian handle it was
    fresh = _env(case, n)
    fresh.rollout(seeds, 150, 20, True, True)
    assert np.array_equal(env.rollout_metrics(), fresh.rollout_metrics())
    env.set_pair_policy(twin.as_state_dict(_weights("init2")))
    env.set_allocator("mlp_coalition")
    with pytest.raises(MuavtaError, match="selected"):
        env.set_pair_policy(None)
    dev = torch.device("cuda", env.device_index)
    with pytest.raises(ValueError, match="shape"):
        env.pair_scores(out={"scores": torch.zeros((n, 16, 32), dtype=torch.float32, device=dev)})
    rings = {k: torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device=dev) for k, (shape, dt) in env.obs_ring_shapes(20).items()}
    with pytest.raises(MuavtaError, match="MLP-Pair"):
        env.rollout_record(seeds, 20, INTERVAL, True, obs_rings=rings)
    env.rollout(seeds, 150, INTERVAL, True, True)
    ref, _ = _policy_env(case, n, "init2")
    ref.rollout(seeds, 150, INTERVAL, True, True)
    assert np.array_equal(env.rollout_metrics(), ref.rollout_metrics())
    env.set_allocator("hungarian")
    env.set_pair_policy(None)                 # NULL clears
    with pytest.raises(MuavtaError, match="set_pair_policy"):
        env.set_allocator("mlp_pair")
    env.rollout(seeds, 150, 20, True, True)
    assert np.array_equal(env.rollout_metrics(), fresh.rollout_metrics())
