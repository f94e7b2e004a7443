"""The wide token pads on the device (MUAVTA_F_TOKEN_PADS: max_tasks = 64, max_agents = 48) for Urgency-Pair, MLP-Pair and MLP-ContextPair:
against the reference's recorded episodes (tools/gen_golden_wide_pads.py), against the host twin of the forward pass (tests/policy_mlp_py.py,
logits bit for bit) and against itself along every path that carries the setting (fused rollout, stepwise allocate, pair_scores ->
allocate_scored, parts, lanes, escalation, policy swaps).  Tolerances: none on logits and on anything between device paths; scores against the
reference's float64 evaluation within 4 x D_ref, D_ref = the reference's own float32 deviation from it, measured on the fixture."""
import os

import numpy as np
import pytest

import policy_mlp_py as twin
import wide_pads as WP
from muavta_amd.native import MuavtaError
from test_gpu_mlp_pair import BOUND, _env, compare_paths, full_state, metrics_of, stepwise

pytestmark = pytest.mark.gpu

MT, MA = WP.MT, WP.MA
WIDE = (MT, MA)
TILE24 = dict(tile_agents=24, tile_tasks=48, tile_threats=24)


def _handle(params, n):
    from muavta_amd.batched import BatchedMultiUAVEnv
    return BatchedMultiUAVEnv(params, n)


def _c_set(env, mt, ma, nbytes=8):
    """muavta_set(MUAVTA_F_TOKEN_PADS) itself, past the Python checks"""
    from muavta_amd.batched import F
    v = np.array([mt, ma], dtype=np.int32)
    return env.L.muavta_set(env.h, F["TOKEN_PADS"], v.ctypes.data, nbytes)


def _urgency(env, pads=WIDE):
    env.set_token_pads(*pads)
    env.set_allocator("urgency_pair")
    return env


def _weights(name, wname):
    return twin.load_weights(WP.LEARNED[name][0], wname)


def _policy_env(case, n, name, wname, pads=WIDE, **kw):
    """a handle with the learned policy `name` ('pair' / 'context') installed from a bare mapping, the pads set by hand"""
    env = _env(case, n, **kw)
    w = _weights(name, wname)
    env.set_token_pads(*pads)
    env.set_pair_policy(twin.as_state_dict(w))
    env.set_allocator("mlp_pair" if name == "pair" else "mlp_context_pair")
    return env, w


def _kind(w):
    return "pair_raw" if w["raw_features"] else "pair"


def _same(a, b, tag):
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), f"{tag}: {k}"


# 6. refusals leave the handle usable
def test_refusals_leave_the_handle_usable():
    import torch
    n, seeds = 4, np.arange(4, dtype=np.uint64)
    small = _env("WPS_hard", n)  # 16 x 40
    assert small.A_tile == 16 and small.token_pads == (32, 16)
    small.set_allocator("urgency_pair")
    with pytest.raises(ValueError, match="tile_agents=24, tile_tasks=48, tile_threats=24"):
        small.set_token_pads(64, 48)
    assert _c_set(small, 64, 48) == -1 and b"tile_agents=24" in small.L.muavta_last_error(small.h)  # the C entry point checks for itself
    with pytest.raises(ValueError, match=r"\(32, 16\) and \(64, 48\)"):
        small.set_token_pads(40, 20)
    assert _c_set(small, 40, 20) == -1 and _c_set(small, 48, 64) == -1 and _c_set(small, 32, 16, nbytes=4) == -1
    assert _c_set(small, 32, 16) == 0
    small.set_token_pads(32, 16)
    small.rollout(seeds, 150, 15, True, True)
    fresh = _urgency(_env("WPS_hard", n), (32, 16))
    fresh.rollout(seeds, 150, 15, True, True)
    assert small.token_pads == (32, 16) and np.array_equal(small.rollout_metrics(), fresh.rollout_metrics())

    env, w = _policy_env("WPS_attn_OS24", n, "pair", "init2")
    env.reset(seeds)
    dev = torch.device("cuda", env.device_index)
    with pytest.raises(ValueError, match=r"\(4, 48, 64\)"):
        env.pair_scores(out={"scores": torch.zeros((n, 16, 32), device=dev)})  # the narrow shape while wide pads are set
    with pytest.raises(ValueError, match=r"\(32, 16\) and \(64, 48\)"):
        env.set_token_pads(64, 16)
    assert env.pair_scores().shape == (n, MA, MT)
    assert tuple(env.get("TOKEN_PADS")) == WIDE
    env.set_token_pads(32, 16)
    assert env.pair_scores().shape == (n, 16, 32)
    with pytest.raises(ValueError, match=r"\(4, 16, 32\)"):
        env.pair_scores(out={"scores": torch.zeros((n, MA, MT), device=dev)})
    env.rollout(seeds, 150, 15, True, True)
    ref, _ = _policy_env("WPS_attn_OS24", n, "pair", "init2", pads=(32, 16))
    ref.rollout(seeds, 150, 15, True, True)
    assert np.array_equal(env.rollout_metrics(), ref.rollout_metrics())


# 7. the default is untouched
@pytest.mark.parametrize("case", ["WPS_escort24", "WPS_burst64"])
@pytest.mark.parametrize("mode", ["urgency_pair", "mlp_pair"])
def test_narrow_pads_after_wide_equal_a_handle_never_touched(case, mode):
    n, steps = 64, 60
    seeds = np.arange(n, dtype=np.uint64) + 7
    states = []
    for touched in (True, False):
        env = _env(case, n)
        if mode == "mlp_pair":
            env.set_pair_policy(twin.as_state_dict(_weights("pair", "init2")))
        if touched:
            env.set_token_pads(64, 48)
            env.set_allocator(mode)
            env.rollout(seeds, 10, 15, True, True)  # the wide kernels ran on this handle
            env.set_token_pads(32, 16)
        env.set_allocator(mode)
        env.rollout(seeds, steps, 15, True, True)
        states.append(full_state(env))
    _same(states[0], states[1], f"{case} {mode}")
    assert states[0]["SCALARS"][:, 23].max() >= 3


# 8. Urgency-Pair at wide pads vs the reference
@pytest.mark.parametrize("path", WP.URG_METRICS, ids=WP.trace_id)
def test_urgency_pair_fused_metrics_vs_reference(path):
    g = np.load(path)
    n = g["metrics"].shape[0]
    env = _urgency(_env(str(g["case"]), n))
    env.rollout(np.arange(n, dtype=np.uint64), 150, 15, True, True)
    assert not env.get("ERROR").any()
    assert np.array_equal(env.rollout_metrics(), g["metrics"]) and np.array_equal(env.get("SCALARS")[:, 23].astype(np.int64), g["n_replans"])


@pytest.mark.parametrize("path", WP.URG_TRACES, ids=WP.trace_id)
def test_urgency_pair_trace_fused_stepwise_and_actions(path):
    """The trace seed: fused metrics and n_replans are the reference's, the stepwise allocate path stages the reference's actions at every
    step; then fused == stepwise full state over 128 envs x 150 steps (an env that outgrows the tile's slots is left out in both alike).
    The > 48 live agents (WPS_burst64) and > 64 underfilled tasks (its derived case) are among the traces."""
    g = np.load(path)
    params = WP.params_of(g)
    seed = np.array([int(g["seed"])], dtype=np.uint64)
    one = _urgency(_handle(params, 1))
    one.rollout(seed, 150, 15, True, True)
    assert not one.get("ERROR").any()
    assert np.array_equal(one.rollout_metrics()[0], g["metrics"]) and int(one.get("SCALARS")[0, 23]) == int(g["n_replans"])
    one.reset(seed)
    for t in range(len(g["replanned"])):
        aa, ai = one.allocate(15, True)
        k = int((aa[0] >= 0).sum())
        order = np.argsort(aa[0, :k], kind="stable")
        assert np.array_equal(np.stack([aa[0, :k][order], ai[0, :k][order]], axis=1), WP.actions_at(g, t).reshape(-1, 2)), f"t={t}: actions vs reference"
        one.step_staged()
    assert np.array_equal(one.metrics()[0], g["metrics"])
    n, steps = 128, 150
    seeds = np.arange(n, dtype=np.uint64) + 100
    fused = _urgency(_handle(params, n))
    fused.rollout(seeds, steps, 15, True, True)
    A = full_state(fused)
    path_b = stepwise(_urgency(_handle(params, n)), seeds, steps, lambda e: e.allocate(15, True, fetch=False))
    full, n_early = compare_paths(str(g["case"]), A, path_b, path_b)
    print(f"{str(g['case'])}: {full} envs compared in full, {n_early} at their earlier end, {n - full - n_early} outgrew the tile")
    assert full + n_early >= 96 and A["SCALARS"][:, 23].max() >= 5


@pytest.mark.parametrize("case,tile", [("WPS_attn_OS24", 24), ("WPS_attn_XL", 64)])
def test_recorded_urgency_pair_rollout_equals_the_fused_one(case, tile):
    """rollout_record in the urgency_pair mode at wide pads runs the recording instantiation of the wide kernel: the final state of every
    env equals the plain fused rollout's, and differs from the recorded rollout at the narrow pads."""
    import torch
    n, steps = 16, 150
    seeds = np.arange(n, dtype=np.uint64) + 30
    fused = _urgency(_env(case, n))
    assert fused.A_tile == tile
    fused.rollout(seeds, steps, 15, True, True)
    A = full_state(fused)
    states = {}
    for pads in (WIDE, (32, 16)):
        rec = _urgency(_env(case, n), pads)
        dev = torch.device("cuda", rec.device_index)
        rings = {k: torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device=dev) for k, (shape, dt) in rec.obs_ring_shapes(steps).items()}
        rec.rollout_record(seeds, steps, 15, True, obs_rings=rings)
        rec.sync()
        states[pads] = full_state(rec)
        assert bool((rings["obs_done"] != 0x80).any().item())  # (MUAVTA_OBS_UNWRITTEN is the pre-fill: the rings were written)
    _same(A, states[WIDE], f"{case}: recorded vs fused")
    assert not A["ERROR"].any() and A["SCALARS"][:, 23].max() >= 5
    assert not np.array_equal(states[WIDE]["metrics"], states[(32, 16)]["metrics"])


# 9. logits, bit for bit against the host twin at 48 x 64
def check_against_twin(env, name, w, tag, rng, per_check):
    """Device logits of every env's current state against the host twin on a sample of the valid cells — a logit is a pure function of its
    pair, so the twin evaluates the sampled cells alone (its numpy chains are what bounds the test's time) — which always holds the
    cells of the wide part of the grid first.  Masked cells are 0, pair_scores is repeatable."""
    kind = WP.LEARNED[name][0]
    tok = env.tokens(_kind(w), MT, MA)
    if name == "context":
        tok = dict(tok, context=env.context(_kind(w), MT))
    scores, logits = env.pair_scores(want_logits=True)
    ev = tok["edge_valid"] != 0
    assert scores.shape == (env.n_envs, MA, MT) and not scores[~ev].any() and not logits[~ev].any(), f"{tag}: masked entries"
    nn, ii, jj = np.nonzero(ev)
    wide = (ii >= 16) | (jj >= 32)
    order = np.concatenate([rng.permutation(np.nonzero(wide)[0]), rng.permutation(np.nonzero(~wide)[0])])[:per_check]
    pick = np.zeros(ev.shape, np.float32)
    pick[nn[order], ii[order], jj[order]] = 1
    ts, tl = twin.forward_batch(kind, w, dict(tok, edge_valid=pick))
    sel = pick != 0
    diff = logits.view(np.uint32)[sel] != tl.view(np.uint32)[sel]
    assert not diff.any(), f"{tag}: {int(diff.sum())} of {int(sel.sum())} logits differ from the host twin"
    assert np.abs(scores.astype(np.float64) - ts)[sel].max(initial=0.0) <= 4 * np.spacing(np.float32(w["score_clamp"])), tag
    assert np.array_equal(env.pair_scores(), scores)
    return int(sel.sum()), int(wide[order].sum())


@pytest.mark.parametrize("name,wname", [("pair", "init2"), ("pair", "init2_raw"), ("context", "init2")])
@pytest.mark.parametrize("case,tile", [("WPS_attn_OS24", 24), ("WPS_attn_XL", 64), ("WPS_burst64", 64)])
def test_logits_equal_the_host_twin_bit_for_bit(case, tile, name, wname):
    """4 envs stepped through their episodes in the mode, checked at t = 0, 1, 2 and every 25th step: up to 600 sampled pairs per check.
    The floors follow from the cases, not from the device: the reference's traces hold about 230 valid pairs per plan on WPS_attn_XL
    (7.6 % of the 3,072 cells) and 37 on WPS_attn_OS24 (1.2 %: 24 agents, at most 15 open tasks, a third of them in rows >= 16), so four
    envs over eight checks offer about 7,000 and 1,200 of which the early, fuller checks are capped at 600: at least 2,500 (1,500 of them in
    the wide part of the grid) on the 64 x 128 tile and 800 (200) on the 24 x 48 tile must have been compared."""
    import torch
    n = 4
    env, w = _policy_env(case, n, name, wname)
    assert env.A_tile == tile
    env.reset(np.arange(n, dtype=np.uint64) + 11)
    rng = np.random.default_rng(5)
    checked = in_wide = 0
    for t in range(150):
        if t < 3 or t % 25 == 0:
            c, wd = check_against_twin(env, name, w, f"{case} {name} {wname} t={t}", rng, 600)
            checked += c; in_wide += wd
        env.allocate(15, True, fetch=False)
        env.step_staged()
    dev = torch.device("cuda", env.device_index)
    out = {"scores": torch.full((n, MA, MT), 7.0, device=dev), "logits": torch.full((n, MA, MT), 7.0, device=dev)}
    env.pair_scores(out=out)
    env.sync()
    s, lg = env.pair_scores(want_logits=True)
    assert np.array_equal(out["scores"].cpu().numpy(), s) and np.array_equal(out["logits"].cpu().numpy(), lg)  # the _device entry equals the host entry
    print(f"{case} {name} {wname}: {checked} logits checked, {in_wide} of them in rows >= 16 or columns >= 32")
    assert not env.get("ERROR").any()
    assert checked >= (800 if tile == 24 else 2500) and in_wide >= (200 if tile == 24 else 1500)


# 10. scores vs the reference, along the reference's trajectory
def replay(name, path):
    """test_gpu_mlp_pair.replay at the wide pads: env 0 follows the reference's episode exactly (allocate_scored fed the fixture's torch
    scores); at every plan the device's tokens (the context kind: and its context) must equal the fixture's and the device's scores are
    compared with the fixture's float64 evaluation.  Returns the worst deviation."""
    g = np.load(path)
    case, wname, interval, seed = str(g["case"]), str(g["weights"]), int(g["interval"]), int(g["seed"])
    env, w = _policy_env(case, 1, name, wname)
    kind = _kind(w)
    env.reset(np.array([seed], dtype=np.uint64))
    worst, k = 0.0, 0
    for t in range(len(g["replanned"])):
        planned = bool(g["replanned"][t])
        sc = np.zeros((1, MA, MT), np.float32)
        if planned:
            assert t == int(g["step"][k])
            tok = env.tokens(kind, MT, MA)
            assert np.array_equal(tok["task_feats"][0], g["tf"][k]) and np.array_equal(tok["agent_feats"][0], g["af"][k]) and np.array_equal(tok["edge_valid"][0], g["ev"][k]), \
                f"{os.path.basename(path)} t={t}: tokens vs reference"
            if name == "context":
                assert np.array_equal(env.context(kind, MT)[0], g["ctx"][k]) and np.array_equal(tok["agent_mask"][0], g["amask"][k]) and np.array_equal(tok["task_mask"][0], g["tmask"][k]), \
                    f"{os.path.basename(path)} t={t}: context / masks vs reference"
            got = env.pair_scores()[0]
            ev = g["ev"][k] != 0
            assert not got[~ev].any()
            if ev.any():
                worst = max(worst, float(np.abs(got.astype(np.float64) - g["scores64"][k])[ev].max()))
            sc[0] = g["scores"][k]
        out = env.allocate_scored(kind, MT, MA, edge_scores=sc, gate="trainer", replan_interval=interval)
        assert bool(out["replanned"][0]) == planned, f"t={t}: gate"
        if planned:
            assert np.array_equal(out["selected"][0], g["selected"][k]), f"t={t}: selected mask vs reference"
            k += 1
        env.step_staged()
    assert k == len(g["step"]) and not env.get("ERROR").any()
    assert np.array_equal(env.metrics()[0], g["metrics"]) and int(env.get("SCALARS")[0, 23]) == int(g["n_replans"])
    return worst


@pytest.mark.parametrize("name,path", WP.ALL_LEARNED_TRACES, ids=WP.trace_id)
def test_scores_vs_reference_along_its_trajectory(name, path):
    D = WP.d_ref(np.load(path))
    worst = replay(name, path)
    print(f"{os.path.basename(path)}: D_ref {D:.3e}, device max |score - scores64| {worst:.3e}, ratio {worst / D:.2f} (bound {BOUND})")
    assert worst <= BOUND * D


# 11. fused == stepwise == scored chain, bit for bit
@pytest.mark.parametrize("interval,use_vis,name,wname", [(15, True, "pair", "init2"), (20, False, "pair", "init2_raw"), (15, False, "context", "init2"), (20, True, "context", "init2")])
@pytest.mark.parametrize("case,tile", [("WPS_attn_OS24", 24), ("WPS_attn_L", 64), ("WPS_attn_XL", 64)])
def test_fused_equals_stepwise_equals_scored_chain(case, tile, interval, use_vis, name, wname):
    """Every env of the batch is compared, none with a tolerance: see test_gpu_mlp_pair.test_fused_equals_stepwise_equals_scored_chain.  The
    chain: pair_scores(out=[n, 48, 64]) feeds allocate_scored(kind, 64, 48, ...) under the plain Hungarian mode.  An env that flags a
    capacity error is left out in all paths alike."""
    import torch
    n, steps = 128, 150
    seeds = np.arange(n, dtype=np.uint64) + 100
    fused, w = _policy_env(case, n, name, wname)
    assert fused.A_tile == tile
    fused.rollout(seeds, steps, interval, use_vis, True)
    rm = fused.rollout_metrics()
    A = full_state(fused)
    assert np.array_equal(A["metrics"], rm)
    step, _ = _policy_env(case, n, name, wname)
    path_b = stepwise(step, seeds, steps, lambda e: e.allocate(interval, use_vis, fetch=False))
    chain, _ = _policy_env(case, n, name, wname)
    chain.set_allocator("hungarian")  # the scores come through the stand-alone kernel: no allocator mode involved
    sc = torch.empty((n, MA, MT), dtype=torch.float32, device=torch.device("cuda", chain.device_index))

    def plan_chain(e):
        e.pair_scores(out={"scores": sc})
        e.allocate_scored(_kind(w), MT, MA, edge_scores=sc, gate="trainer", replan_interval=interval, use_visibility=use_vis, edge_valid_only=True, out={})
    full, n_early = compare_paths(case, A, path_b, stepwise(chain, seeds, steps, plan_chain))
    print(f"{case} {name} {wname} interval {interval} vis {use_vis}: {n} envs, {full} compared in full at step {steps}, {n_early} at their earlier end, "
          f"{n - full - n_early} outgrew the tile")
    assert full + n_early >= 96, f"{full + n_early} of {n} envs compared"
    assert A["SCALARS"][:, 23].max() >= 5  # plans were made


# 12. episodes vs the reference
@pytest.mark.parametrize("name", ["pair", "context"])
def test_fused_episodes_vs_reference(name):
    """Fused metrics and n_replans of every recorded episode against the reference's two columns: metrics32 (the policy's own float32
    scores) and metrics64 (scores64 cast to float32).  A last-bit difference in a score can flip a near-tie, after which the episode
    diverges, so the cap follows the reference's own behaviour: with F_ref = the episodes whose float32 and float64 columns differ, at
    most E / 10 + F_ref episodes of the E recorded (weight set init2 under the wps_eval loop) may equal neither column; every other one
    equals one of them bit for bit.  (For MLP-ContextPair the reference's F_ref is 5 of 48, above the E / 10 the issue hoped for — see
    tools/gen_golden_wide_pads.py —; the rule and its cap are applied to that kind as they stand.)"""
    paths = WP.LEARNED_METRICS[name]
    assert len(paths) == 3
    E = F = 0
    neither, only64 = [], []
    for p in paths:
        g = np.load(p)
        case, n = str(g["case"]), g["metrics32"].shape[0]
        F += sum(not (np.array_equal(a, b) and ra == rb) for a, b, ra, rb in zip(g["metrics32"], g["metrics64"], g["n_replans32"], g["n_replans64"]))
        E += n
        env, _ = _policy_env(case, n, name, "init2")
        env.rollout(g["seeds"].astype(np.uint64), 150, 15, True, True)
        got, reps = env.rollout_metrics(), env.get("SCALARS")[:, 23].astype(np.int64)
        assert not env.get("ERROR").any()
        for s in range(n):
            is32 = np.array_equal(got[s], g["metrics32"][s]) and reps[s] == g["n_replans32"][s]
            is64 = np.array_equal(got[s], g["metrics64"][s]) and reps[s] == g["n_replans64"][s]
            if not is32 and not is64:
                neither.append((case, int(g["seeds"][s])))
            elif not is32:
                only64.append((case, int(g["seeds"][s])))
    cap = E / 10 + F
    print(f"{name}: E = {E}, F_ref = {F}; the device equals neither column in {len(neither)} episodes {neither} (cap {cap}), the float64 column alone in {len(only64)} {only64}")
    assert E >= 48 and len(neither) <= cap, neither


# 13. parts, lanes, escalation, policy swap at wide pads
def test_parts_lanes_escalation_and_policy_swap():
    case, n = "WPS_attn_OS24", 128
    sets = [np.arange(k * 1000, k * 1000 + n, dtype=np.uint64) for k in range(2)]
    one, _ = _policy_env(case, n, "pair", "init2")
    one.set_lanes(1)
    want = []
    for sd in sets:
        one.rollout(sd, 150, 15, True, True)
        one.sync()
        want.append(one.rollout_metrics())
    err = one.get("ERROR")
    # two seeded batches back to back on two lanes; the second lane is created AFTER the pads, the policy and the mode were set
    two, _ = _policy_env(case, n, "pair", "init2")
    two.set_lanes(2)
    for sd in sets:
        two.rollout(sd, 150, 15, True, True)
    assert np.array_equal(two.rollout_metrics(back=1), want[0]) and np.array_equal(two.rollout_metrics(), want[1])
    # pads set while both lanes exist reach both: narrow on both, then wide again
    narrow, _ = _policy_env(case, n, "pair", "init2", pads=(32, 16))
    narrow.rollout(sets[0], 150, 15, True, True)
    two.set_token_pads(32, 16)
    for sd in (sets[0], sets[0]):
        two.rollout(sd, 150, 15, True, True)
    assert np.array_equal(two.rollout_metrics(back=1), narrow.rollout_metrics()) and np.array_equal(two.rollout_metrics(), narrow.rollout_metrics())
    assert not np.array_equal(narrow.rollout_metrics(), want[0])
    two.set_token_pads(64, 48)
    # policy swaps between rollouts: Pair -> ContextPair -> Coalition -> Pair, each equal to a fresh handle's
    w_co = twin.load_weights(twin.COALITION, "init2")
    fresh_ctx, w_ctx = _policy_env(case, n, "context", "init2")
    fresh_ctx.rollout(sets[0], 150, 15, True, True)
    fresh_co = _env(case, n)
    fresh_co.set_pair_policy(twin.as_checkpoint(w_co))
    fresh_co.set_allocator("mlp_coalition")
    fresh_co.rollout(sets[0], 150, 12, True, True)
    two.set_pair_policy(twin.as_state_dict(w_ctx))
    two.rollout(sets[0], 150, 15, True, True)
    assert np.array_equal(two.rollout_metrics(), fresh_ctx.rollout_metrics()) and two.pair_scores().shape == (n, MA, MT)
    two.set_pair_policy(twin.as_checkpoint(w_co))  # MLP-Coalition keeps its own 16 x 48 grid, whatever the pads
    two.rollout(sets[0], 150, 12, True, True)
    assert np.array_equal(two.rollout_metrics(), fresh_co.rollout_metrics()) and two.pair_scores().shape == (n, 16, 48) and two.token_pads == WIDE
    two.set_pair_policy(twin.as_state_dict(_weights("pair", "init2")))
    two.rollout(sets[1], 150, 15, True, True)
    assert np.array_equal(two.rollout_metrics(), want[1])
    # sub-batches
    parts, _ = _policy_env(case, n, "pair", "init2")
    parts.reset(sets[0])
    parts.set_parts(2)
    for p in range(2):
        parts.rollout_part(p, 150, 15, True, True)
    parts.sync()
    assert np.array_equal(metrics_of(parts), want[0])
    parts.reset(sets[1])
    for t in range(150):
        for p in range(2):
            parts.allocate_part(p, 15, True, fetch=False)
            parts.step_part(p, None, None)
    parts.sync()
    by_parts = metrics_of(parts)
    parts.set_parts(0)
    step, _ = _policy_env(case, n, "pair", "init2")
    step.reset(sets[1])
    for t in range(150):
        step.allocate(15, True, fetch=False); step.step_staged()
    assert np.array_equal(by_parts, metrics_of(step))
    assert np.array_equal(err, step.get("ERROR")) and (err == 0).sum() >= 96
    # escalation from the capped 24 x 48 tile to 64 x 128: the escalated handle carries the pads, its rows equal a direct rollout there
    for name in ("pair", "context"):
        small, _ = _policy_env(case, 64, name, "init2")
        small.set_slot_cap(24)
        seeds = np.arange(500, 564, dtype=np.uint64)
        small.rollout(seeds, 150, 15, True, True, escalate=True)
        assert len(small.escalated) > 0 and all(h.A_tile == 64 and h.token_pads == WIDE for h, _ in small.escalated.values())
        got = small.rollout_metrics()
        big, _ = _policy_env(case, 64, name, "init2", tile_agents=64, tile_tasks=128, tile_threats=48)
        big.rollout(seeds, 150, 15, True, True)
        assert np.array_equal(got, big.rollout_metrics())
    urg = _urgency(_env(case, 64))
    urg.set_slot_cap(24)
    urg.rollout(seeds, 150, 15, True, True, escalate=True)
    assert len(urg.escalated) > 0 and all(h.token_pads == WIDE for h, _ in urg.escalated.values())
    big = _urgency(_env(case, 64, tile_agents=64, tile_tasks=128, tile_threats=48))
    big.rollout(seeds, 150, 15, True, True)
    assert np.array_equal(urg.rollout_metrics(), big.rollout_metrics())
