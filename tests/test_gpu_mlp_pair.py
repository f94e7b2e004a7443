"""The learned MLP-Pair hybrid on the device (MUAVTA_ALLOC_MLP_PAIR, csrc/sim/policy.inc) against its host twin (tests/policy_mlp_py.py:
the arithmetic contract, bit for bit up to the logits), against the reference's recorded episodes (tools/gen_golden_mlp_pair.py) and
against itself along every path that carries the mode (fused rollout, stepwise allocate, pair_scores -> allocate_scored, parts, lanes,
escalation).  Tolerances: none on logits and on anything between device paths; scores against the reference's float64 evaluation within
4 x D_ref, D_ref = the reference's own float32 deviation from that evaluation, measured on the fixtures (never on the device)."""
import glob
import os

import numpy as np
import pytest

import policy_mlp_py as twin
from muavta_amd.native import MuavtaError
from muavta_amd.params import params_for_case
from test_gpu_parity import Snapshot

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TRACES = sorted(glob.glob(os.path.join(GOLDEN, "mlppair_trace_*.npz")))
METRICS = sorted(glob.glob(os.path.join(GOLDEN, "mlppair_metrics_*.npz")))
TILE_CASES = [("WPS_hard", 16), ("WPS_escort24", 24), ("WPS_burst64", 64)]
BOUND = 4.0  # x D_ref


def _env(case, n, **kw):
    from muavta_amd.batched import BatchedMultiUAVEnv
    return BatchedMultiUAVEnv(params_for_case(case, **kw), n)


def _weights(name):
    return twin.load_weights(twin.PAIR, name)


def _policy_env(case, n, wname, **kw):
    env = _env(case, n, **kw)
    w = _weights(wname)
    env.set_pair_policy(twin.as_state_dict(w))
    env.set_allocator("mlp_pair")
    return env, w


def _kind(w):
    return "pair_raw" if w["raw_features"] else "pair"


def d_ref_of(wname):
    """max |scores - scores64| of the reference over every recorded trace of this weight set"""
    worst = 0.0
    for p in TRACES:
        g = np.load(p)
        if str(g["weights"]) == wname:
            ev = g["ev"] != 0
            worst = max(worst, float(np.abs(g["scores"].astype(np.float64) - g["scores64"])[ev].max()))
    assert worst > 0
    return worst


def check_against_twin(env, w, tag):
    tok = env.tokens(_kind(w), 32, 16)
    scores, logits = env.pair_scores(want_logits=True)
    ts, tl = twin.forward_batch(twin.PAIR, w, tok)
    ev = tok["edge_valid"] != 0
    assert np.array_equal(logits.view(np.uint32), tl.view(np.uint32)), f"{tag}: {int((logits.view(np.uint32) != tl.view(np.uint32)).sum())} of {int(ev.sum())} logits differ from the host twin"
    assert not scores[~ev].any() and not logits[~ev].any(), f"{tag}: masked entries"
    # tanhf against numpy's float32 tanh: a few ulp of the score range
    assert np.abs(scores.astype(np.float64) - ts)[ev].max(initial=0.0) <= 4 * np.spacing(np.float32(w["score_clamp"])), tag
    assert np.array_equal(env.pair_scores(), scores)
    return int(ev.sum())


# 4. logits, bit for bit
@pytest.mark.parametrize("wname", ["init2", "init2_raw", "il3"])
@pytest.mark.parametrize("case,tile", TILE_CASES)
def test_logits_equal_the_host_twin_bit_for_bit(case, tile, wname):
    n = 8
    env, w = _policy_env(case, n, wname)
    assert env.A_tile == tile
    env.reset(np.arange(n, dtype=np.uint64) + 11)
    checked = 0
    for t in range(150):
        if t < 3 or t % 7 == 0:
            checked += check_against_twin(env, w, f"{case} {wname} t={t}")
        env.allocate(15, True, fetch=False)
        env.step_staged()
    checked += check_against_twin(env, w, f"{case} {wname} end")
    assert checked > 2000 and not env.get("ERROR").any()


def test_pair_scores_device_tensors_equal_the_host_path():
    import torch
    n = 64
    env, w = _policy_env("WPS_hard_x2", n, "init2")
    env.reset(np.arange(n, dtype=np.uint64))
    for _ in range(20):
        env.allocate(15, True, fetch=False); env.step_staged()
    dev = torch.device("cuda", env.device_index)
    out = {"scores": torch.full((n, 16, 32), 7.0, device=dev), "logits": torch.full((n, 16, 32), 7.0, device=dev)}
    env.pair_scores(out=out)
    env.sync()
    s, lg = env.pair_scores(want_logits=True)
    assert np.array_equal(out["scores"].cpu().numpy(), s) and np.array_equal(out["logits"].cpu().numpy(), lg)
    with pytest.raises(ValueError):
        env.pair_scores(out={"scores": torch.zeros((n, 16, 31), device=dev)})
    with pytest.raises(ValueError):
        env.pair_scores(out={"scores": torch.zeros((n, 16, 32), dtype=torch.int32, device=dev)})
    with pytest.raises(ValueError):
        env.pair_scores(out={})


def test_tanhf_over_its_range():
    """The recorded weight sets keep the logits within about +-1, where tanh is nearly linear.  Here layer 3 of init2 is scaled by 8
    (logits to beyond +-4): logits still bit for bit against the host twin, scores against tanh of the SAME logit evaluated in float64,
    times score_clamp.  Bound: 4 spacings of score_clamp = 5.7 ulp of a tanh value near 1 scaled by 0.35 — the 5 ulp OpenCL allows a
    float tanh plus the half ulp of the multiplication (the issue reckons with about two ulp)."""
    n = 64
    w = _weights("init2")
    w["w2"], w["b2"] = (w["w2"] * np.float32(8)).astype(np.float32), (w["b2"] * np.float32(8)).astype(np.float32)
    env = _env("WPS_hard_x2", n)
    env.set_pair_policy(twin.as_state_dict(w))
    env.set_allocator("mlp_pair")
    env.reset(np.arange(n, dtype=np.uint64) + 40)
    lo, hi, worst = 0.0, 0.0, 0.0
    for t in range(60):
        if t % 6 == 0:
            tok = env.tokens("pair", 32, 16)
            scores, logits = env.pair_scores(want_logits=True)
            _, tl = twin.forward_batch(twin.PAIR, w, tok)
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


# 5. scores vs the reference, along the reference's trajectory
def replay(path, tile_kw=None):
    """env 0 follows the reference's episode exactly (allocate_scored fed the fixture's torch scores); at every plan the device's tokens
    must equal the fixture's and the device's scores are compared with the fixture's float64 evaluation.  Returns the worst deviation."""
    g = np.load(path)
    case, wname, interval, seed = str(g["case"]), str(g["weights"]), int(g["interval"]), int(g["seed"])
    env, w = _policy_env(case, 1, wname, **(tile_kw or {}))
    kind = _kind(w)
    env.reset(np.array([seed], dtype=np.uint64))
    worst, k = 0.0, 0
    for t in range(len(g["replanned"])):
        planned = bool(g["replanned"][t])
        sc = np.zeros((1, 16, 32), np.float32)
        if planned:
            assert t == int(g["step"][k])
            tok = env.tokens(kind, 32, 16)
            assert np.array_equal(tok["task_feats"][0], g["tf"][k]) and np.array_equal(tok["agent_feats"][0], g["af"][k]) and np.array_equal(tok["edge_valid"][0], g["ev"][k]), \
                f"{os.path.basename(path)} t={t}: tokens vs reference"
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
    return worst, wname


@pytest.mark.parametrize("path", TRACES, ids=lambda p: os.path.basename(p)[:-4])
def test_scores_vs_reference_along_its_trajectory(path):
    g = np.load(path)
    ev = g["ev"] != 0
    D = float(np.abs(g["scores"].astype(np.float64) - g["scores64"])[ev].max())
    worst, _ = replay(path)
    print(f"{os.path.basename(path)}: D_ref {D:.3e}, device max |score - scores64| {worst:.3e}, ratio {worst / D:.2f} (bound {BOUND})")
    assert worst <= BOUND * D


# 6. the chain, bit for bit
def metrics_of(env):
    """muavta_metrics of every env; a capacity flag somewhere in the batch (MUAVTA_E_CAPACITY: the rows are filled all the same) is the
    caller's to handle through ERROR"""
    m = np.empty((env.n_envs, 30), dtype=np.float64)
    rc = env.L.muavta_metrics(env.h, m.ctypes.data)
    assert rc in (0, -4), env.L.muavta_last_error(env.h)
    return m


def full_state(env):
    s = Snapshot(env)
    d = {n: getattr(s, n) for n in Snapshot.NAMES}
    d["metrics"] = metrics_of(env)
    return d


def assert_same(a, b, rows, tag):
    for k in a:
        assert np.array_equal(np.asarray(a[k])[rows], np.asarray(b[k])[rows]), f"{tag}: {k}"


def stepwise(env, seeds, steps, plan):
    """`plan(env)` then step_staged, `steps` times -> (full state, which envs' episodes ended before the last step, what those held when they ended)"""
    n = len(seeds)
    env.reset(seeds)
    early = np.zeros(n, bool)
    at_end = {}  # env -> (metrics row, SCALARS row, ERROR) when its episode ended before the last step
    for t in range(steps):
        plan(env)
        env.step_staged()
        if t < steps - 1:
            _, term, trunc = env.step_result()
            new = ((term != 0) | (trunc != 0)) & ~early
            if new.any():
                m, sc, er = metrics_of(env), env.get("SCALARS"), env.get("ERROR")
                for i in np.nonzero(new)[0]:
                    at_end[int(i)] = (m[i].copy(), sc[i].copy(), int(er[i]))
                early |= new
    return full_state(env), early, at_end


def compare_paths(case, A, path_b, path_c):
    """fused state A against the two stepwise paths (each what `stepwise` returned), bit for bit -> (envs compared in full at the last step, envs
    compared at their earlier end).  An env that flagged a capacity error holds no result and is left out, in every path alike."""
    (B, early, endB), (Cc, early_c, endC) = path_b, path_c
    assert np.array_equal(early, early_c) and np.array_equal(B["ERROR"], Cc["ERROR"])
    ok = (A["ERROR"] == 0) & (B["ERROR"] == 0)
    assert np.array_equal(A["ERROR"][~early] != 0, B["ERROR"][~early] != 0)
    assert_same(B, Cc, ok, f"{case} stepwise vs scored chain")
    assert_same(A, B, ok & ~early, f"{case} fused vs stepwise")
    n_early = 0
    for i in np.nonzero(early)[0]:
        mb, sb, eb = endB[int(i)]
        mc, scc, ec = endC[int(i)]
        assert eb == ec and np.array_equal(mb, mc) and np.array_equal(sb, scc), f"{case} env {i}: stepwise vs scored chain at the episode's end"
        if eb == 0 and A["ERROR"][i] == 0:
            assert np.array_equal(A["metrics"][i], mb) and np.array_equal(A["SCALARS"][i], sb), f"{case} env {i}: fused vs stepwise at the episode's end"
            n_early += 1
    return int((ok & ~early).sum()), n_early


@pytest.mark.parametrize("interval,use_vis,wname", [(15, True, "init2"), (20, False, "init2_raw"), (20, True, "il3"), (15, False, "init2_raw")])
@pytest.mark.parametrize("case,tile", TILE_CASES)
def test_fused_equals_stepwise_equals_scored_chain(case, tile, interval, use_vis, wname):
    """Every env of the batch is compared, none with a tolerance.  An env that runs to the last step: every field of the state, the
    metrics and n_replans, fused == stepwise == scored chain.  An env whose episode ends earlier: the fused loop stops stepping it there
    while the stepwise loops (like four separate calls on the reference) keep stepping it, so its fused final rows are compared with what
    the stepwise paths held at the step it ended.  An env that outgrows its tile (the 24-agent escort case holds more pending reveals
    than its tile under a churning policy) stops with ERROR set in every path alike and holds no result; the batch is sized so that at
    least 256 envs per tile stay within it."""
    import torch
    n, steps = (256 if tile == 16 else 384), 150
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
    assert compared >= 256, f"{compared} of {n} envs compared"
    assert A["SCALARS"][:, 23].max() >= 5  # plans were made
    if tile == 16:
        assert not A["ERROR"].any() and compared == n


def test_parts_lanes_escalation_and_policy_swap():
    case, n = "WPS_hard_x2", 256
    sets = [np.arange(k * 1000, k * 1000 + n, dtype=np.uint64) for k in range(2)]
    one, _ = _policy_env(case, n, "init2")
    one.set_lanes(1)
    want = []
    for sd in sets:
        one.rollout(sd, 150, 15, True, True)
        one.sync()
        want.append(one.rollout_metrics())
        assert not one.get("ERROR").any()
    # two seeded batches back to back on two lanes; the second lane is created AFTER the policy and the mode were set
    two, _ = _policy_env(case, n, "init2")
    two.set_lanes(2)
    for sd in sets:
        two.rollout(sd, 150, 15, True, True)
    assert np.array_equal(two.rollout_metrics(back=1), want[0]) and np.array_equal(two.rollout_metrics(), want[1])
    # a second set_pair_policy between rollouts reaches both lanes; setting the first one again restores the first results
    w_il = _weights("il3")
    ref_il, _ = _policy_env(case, n, "il3")
    ref_il.rollout(sets[0], 150, 15, True, True)
    two.set_pair_policy(twin.as_state_dict(w_il))
    for sd in (sets[0], sets[0]):
        two.rollout(sd, 150, 15, True, True)
    assert np.array_equal(two.rollout_metrics(back=1), ref_il.rollout_metrics()) and np.array_equal(two.rollout_metrics(), ref_il.rollout_metrics())
    assert not np.array_equal(ref_il.rollout_metrics(), want[0])
    two.set_pair_policy(twin.as_state_dict(_weights("init2")))
    two.rollout(sets[1], 150, 15, True, True)
    assert np.array_equal(two.rollout_metrics(), want[1])
    # sub-batches
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
    # escalation on a capped tile: flagged envs get the larger tile's row, equal to a direct rollout there
    small, _ = _policy_env(case, 64, "init2")
    small.set_slot_cap(20)
    seeds = np.arange(500, 564, dtype=np.uint64)
    small.rollout(seeds, 150, 15, True, True, escalate=True)
    assert len(small.escalated) > 0 and all(h.A_tile == 24 for h, _ in small.escalated.values())
    got = small.rollout_metrics()
    big, _ = _policy_env(case, 64, "init2", tile_agents=24, tile_tasks=48, tile_threats=24)
    big.rollout(seeds, 150, 15, True, True)
    assert np.array_equal(got, big.rollout_metrics())


# 7. episodes vs the reference
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
    columns differ, at most max(2, 2 x F_ref) episodes of the 48 recorded for weight set init2 under the wps_eval loop may differ, every
    other one is equal bit for bit; the two 8-episode groups (raw features, the trained set; interval 20) get 2 x F_ref = 0.
    DEPARTURE from the issue: it asks for a differing episode to be replayed along the REFERENCE's trajectory as in test 5 up to its first
    differing plan; the fixtures hold one full trace per case, not one per metrics seed, so a differing episode is instead
    replayed stepwise on the device in the mode: along it — up to and beyond the plan at which it leaves the reference's trajectory —
    every plan's scores stay within 4 x D_ref of the float64 evaluation of the same net on the device's own tokens (which are bit-exact
    restatements of the reference's), i.e. what differs is a near-tie, not a score."""
    wname, interval = key
    w = _weights(wname)
    D = d_ref_of(wname)
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
    cap = max(2, 2 * F) if E >= 48 else 2 * F  # (the floor of 2 belongs to the issue's E >= 48 episodes: a small group gets no allowance of its own)
    print(f"{wname} interval {interval}: E = {E}, F_ref = {F}, device differs in {len(differing)} episodes {differing} (cap {cap})")
    assert len(differing) <= cap, differing
    for case, s in differing:
        env, _ = _policy_env(case, 1, wname)
        env.reset(np.array([s], dtype=np.uint64))
        worst = 0.0
        for t in range(150):
            tok = env.tokens(_kind(w), 32, 16)
            got = env.pair_scores()[0]
            s64, _ = twin.forward64(twin.PAIR, w, {k: v[0] for k, v in tok.items()})
            ev = tok["edge_valid"][0] != 0
            if ev.any():
                worst = max(worst, float(np.abs(got.astype(np.float64) - s64)[ev].max()))
            env.allocate(interval, True, fetch=False)
            env.step_staged()
        print(f"  {case} seed {s}: max |score - scores64| along the episode {worst:.3e} = {worst / D:.2f} x D_ref")
        assert worst <= BOUND * D, (case, s)


# 8. refusals
def test_refusals_leave_the_handle_usable():
    import torch
    case, n = "WPS_hard", 4
    env = _env(case, n)
    seeds = np.arange(n, dtype=np.uint64)
    with pytest.raises(MuavtaError, match="set_pair_policy"):
        env.set_allocator("mlp_pair")
    env.reset(seeds)
    with pytest.raises(MuavtaError, match="no policy"):
        env.pair_scores()
    w = _weights("init2")
    with pytest.raises(ValueError, match="use_attention"):
        env.set_pair_policy({"state_dict": {}, "use_attention": True})
    bad = twin.as_state_dict(w)
    bad["pair_mlp.0.weight"] = np.zeros((128, 24), np.float32)
    with pytest.raises(ValueError, match="pair_mlp.0.weight"):
        env.set_pair_policy(bad)
    # the C entry point checks for itself
    from muavta_amd import native
    import ctypes as C
    z = np.zeros(128 * 128, np.float32)
    spec = native.MuavtaPairMlp(0, 64, 0.35, *([z.ctypes.data] * 6))
    assert env.L.muavta_set_pair_policy(env.h, C.byref(spec)) == -1 and b"hidden" in env.L.muavta_last_error(env.h)
    env.rollout(seeds, 150, 20, True, True)   # still the Hungarian handle it was
    fresh = _env(case, n)
    fresh.rollout(seeds, 150, 20, True, True)
    assert np.array_equal(env.rollout_metrics(), fresh.rollout_metrics())
    env.set_pair_policy(twin.as_state_dict(w))
    env.set_allocator("mlp_pair")
    with pytest.raises(MuavtaError, match="selected"):
        env.set_pair_policy(None)
    dev = torch.device("cuda", env.device_index)
    rings = {k: torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device=dev) for k, (shape, dt) in env.obs_ring_shapes(20).items()}
    with pytest.raises(MuavtaError, match="MLP-Pair"):
        env.rollout_record(seeds, 20, 15, True, obs_rings=rings)
    env.rollout(seeds, 150, 15, True, True)
    ref, _ = _policy_env(case, n, "init2")
    ref.rollout(seeds, 150, 15, True, True)
    assert np.array_equal(env.rollout_metrics(), ref.rollout_metrics())
    env.set_allocator("hungarian")
    env.set_pair_policy(None)
    with pytest.raises(MuavtaError, match="set_pair_policy"):
        env.set_allocator("mlp_pair")
    env.rollout(seeds, 150, 20, True, True)
    assert np.array_equal(env.rollout_metrics(), fresh.rollout_metrics())
