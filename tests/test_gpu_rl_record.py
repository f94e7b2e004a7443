"""The RL transitions of the learned pair policies recorded inside the fused rollout (MuavtaRlRings of muavta_rollout_record,
`rollout_rl_record` / `il.rl_record`) against the gate-by-gate loop it replaces (`il.rl_run_stream`), against the host twin of the forward
pass (tests/policy_mlp_py.py) and against the plain rollout.  Everything is compared bit for bit except the noisy scores, whose tanhf is
held to the bound of test_gpu_mlp_pair.test_tanhf_over_its_range (4 spacings of score_clamp; derivation there)."""
import ctypes as C

import numpy as np
import pytest

import policy_mlp_py as twin
from muavta_amd import il
from muavta_amd.native import MuavtaError
from muavta_amd.params import MuavtaRecord, MuavtaRlRings, params_for_case
from test_gpu_parity import Snapshot

pytestmark = pytest.mark.gpu

TILE_CASES = [("WPS_hard", 16), ("WPS_escort24", 24), ("WPS_burst64", 64)]
KINDS = {"pair": twin.PAIR, "context": twin.CONTEXT}
TOK = ("task_feats", "task_mask", "agent_feats", "agent_mask", "edge_valid")
CANARY = 77


def _env(case, n, kind, wname, params=None, **kw):
    from muavta_amd.batched import BatchedMultiUAVEnv
    env = BatchedMultiUAVEnv(params if params is not None else params_for_case(case, **kw), n)
    w = twin.load_weights(KINDS[kind], wname)
    env.set_pair_policy(twin.as_state_dict(w))
    env.set_allocator("mlp_pair")
    return env, w


def _tok_kind(w):
    return "pair_raw" if w["raw_features"] else "pair"


def _alloc(env, G, fill=None):
    import torch
    dev = torch.device("cuda", env.device_index)
    tdt = {np.float32: torch.float32, np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64}
    mk = (lambda s, d: torch.empty(s, dtype=tdt[d], device=dev)) if fill is None else (lambda s, d: torch.full(s, fill, dtype=tdt[d], device=dev))
    return {name: mk(shape, dtype) for name, (shape, dtype) in env.rl_record_shapes(G).items()}


def record(env, seeds, n_steps, interval, G, noise=None, use_vis=True):
    """one rollout_rl_record launch -> the rings as numpy arrays"""
    rings = _alloc(env, G)
    env.rollout_rl_record(seeds, n_steps, interval, use_vis, rings, noise=noise, write_obs=True)
    env.sync()
    out = {k: v.cpu().numpy() for k, v in rings.items()}
    if noise is not None:
        out["noise"] = noise.cpu().numpy()
    return out


def state_of(env):
    s = Snapshot(env)
    d = {n: getattr(s, n) for n in Snapshot.NAMES}
    d["obs"], d["reward"], d["term"], d["trunc"] = s.obs, s.reward, s.term, s.trunc
    d["rollout_metrics"] = env.rollout_metrics()
    return d


def assert_state_equal(a, b, tag):
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, dict):  # (the observation)
            assert all(np.array_equal(x[f], y[f], equal_nan=x[f].dtype.kind == "f") for f in x), f"{tag}: {k}"
        else:
            assert np.array_equal(x, y, equal_nan=np.asarray(x).dtype.kind == "f"), f"{tag}: {k}"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def gate_loop(case, n, kind, wname, seeds, interval, use_vis, max_launches, scores_for=None, params=None):
    """env B: il.rl_run_stream with the trainer's gate and the flags of MUAVTA_ALLOC_MLP_PAIR's plan; its policy returns B's own
    pair_scores, or scores_for(gate ordinal of every env) -> [N, 16, 32].  max_steps = 1: one env step per launch, so that the context
    vector can be read at the same points too.  -> per env the list of its transitions, one per launch in which `replanned` is 1."""
    import torch
    B, w = _env(case, n, kind, wname, params=params)
    dev = torch.device("cuda", B.device_index)
    sc = torch.zeros((n, 16, 32), dtype=torch.float32, device=dev)
    ordinal = np.zeros(n, dtype=np.int64)
    is_ctx = kind == "context"
    ctx_now = {}

    def policy(tok):
        if is_ctx:
            ctx_now["v"] = B.context(_tok_kind(w), 32)
        if scores_for is None:
            B.pair_scores(out={"scores": sc})
        else:
            sc.copy_(torch.from_numpy(scores_for(ordinal)).to(dev))
            torch.cuda.synchronize(dev)
        return sc

    per_env = [[] for _ in range(n)]
    for _, tr in il.rl_run_stream(B, seeds, policy, interval=interval, kind=_tok_kind(w), max_tasks=32, max_agents=16, gate="trainer",
                                  max_steps=1, max_launches=max_launches, use_visibility=use_vis):
        rp = tr["replanned"].cpu().numpy()
        if not rp.any():
            continue
        host = {"tok": {k: tr["tok"][k].cpu().numpy() for k in TOK}, "next_tok": {k: tr["next_tok"][k].cpu().numpy() for k in TOK},
                "scores": tr["scores"].cpu().numpy(), "selected": tr["selected"].cpu().numpy(), "s_wps": tr["s_wps"].cpu().numpy(),
                "done": tr["done"].cpu().numpy()}
        ctx_next = B.context(_tok_kind(w), 32) if is_ctx else None
        for e in np.nonzero(rp)[0]:
            row = {"scores": host["scores"][e], "selected": host["selected"][e], "before": host["s_wps"][0, e], "after": host["s_wps"][1, e], "done": host["done"][e]}
            row.update({k: host["tok"][k][e] for k in TOK})
            row.update({"next_" + k: host["next_tok"][k][e] for k in TOK})
            if is_ctx:
                row["context"], row["next_context"] = ctx_now["v"][e], ctx_next[e]
            per_env[e].append(row)
        ordinal += rp != 0
    return per_env


def assert_slots_equal_loop(A, per_env, tag, with_scores=True):
    G, n = A["step"].shape
    total = 0
    for e in range(n):
        rows = per_env[e]
        assert A["n_gates"][e] == len(rows), f"{tag} env {e}: {A['n_gates'][e]} gates recorded, {len(rows)} launches planned"
        for k, row in enumerate(rows[:G]):
            assert A["step"][k, e] >= 0
            names = [n_ for n_ in row if n_ not in ("before", "after", "scores")] + (["scores"] if with_scores else [])
            for name in names:
                assert np.array_equal(bits(A[name][k, e]), bits(row[name])), f"{tag} env {e} slot {k}: {name}"
            assert bits(A["s_wps_before"][k, e]) == bits(np.float64(row["before"])) and bits(A["s_wps_after"][k, e]) == bits(np.float64(row["after"])), f"{tag} env {e} slot {k}: S_WPS"
            total += 1
        assert (A["step"][len(rows):, e] == -1).all()
    return total


# 3. fused rings = the gate-by-gate loop; final state = the plain rollout
@pytest.mark.parametrize("kind", ["pair", "context"])
@pytest.mark.parametrize("wname", ["init2", "init2_raw", "il3"])
@pytest.mark.parametrize("case,tile", TILE_CASES)
def test_rings_equal_the_gate_by_gate_loop(case, tile, wname, kind):
    n, steps, interval, G = 8, 150, 20, 64
    seeds = np.arange(n, dtype=np.uint64) + 300
    A, w = _env(case, n, kind, wname)
    assert A.A_tile == tile
    rings = record(A, seeds, steps, interval, G)
    assert rings["n_gates"].min() >= 1
    total = assert_slots_equal_loop(rings, gate_loop(case, n, kind, wname, seeds, interval, True, steps), f"{case} {wname} {kind}")
    written = rings["step"] >= 0
    masked = rings["edge_valid"][written] == 0
    assert not rings["scores"][written][masked].any() and not rings["logits"][written][masked].any()
    plain, _ = _env(case, n, kind, wname)
    plain.rollout(seeds, steps, interval, True, True)
    assert_state_equal(state_of(A), state_of(plain), f"{case} {wname} {kind}: final state against the plain rollout")
    print(f"{case} {wname} {kind}: {total} transitions equal the loop's, n_gates {rings['n_gates'].tolist()}")


# 4. logits against the host twin, over every written slot
@pytest.mark.parametrize("kind,wname", [("pair", "init2"), ("pair", "init2_raw"), ("context", "il3"), ("context", "init2_raw")])
def test_recorded_logits_equal_the_host_twin(kind, wname):
    n, steps, G = 8, 45, 45
    env, w = _env("WPS_hard", n, kind, wname)
    rings = record(env, np.arange(n, dtype=np.uint64) + 11, steps, 20, G)
    written = rings["step"] >= 0
    assert written.sum() >= 3 * n and (rings["n_gates"] <= G).all()
    tok = {k: rings[k][written] for k in TOK + (("context",) if kind == "context" else ())}
    ts, tl = twin.forward_batch(KINDS[kind], w, tok)
    assert np.array_equal(bits(rings["logits"][written]), bits(tl))
    assert np.abs(rings["scores"][written].astype(np.float64) - ts).max() <= 4 * np.spacing(np.float32(w["score_clamp"]))
    assert (tok["edge_valid"] != 0).sum() > 1000


# 5. exploration noise
@pytest.mark.parametrize("kind,wname", [("pair", "init2"), ("context", "init2")])
def test_noise(kind, wname):
    import torch
    case, n, steps, interval, G = "WPS_hard", 16, 150, 20, 150  # (a slot for every step: every gate is recorded)
    seeds = np.arange(n, dtype=np.uint64) + 500
    A, w = _env(case, n, kind, wname)
    dev = torch.device("cuda", A.device_index)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    noise = torch.randn((G, n, 16, 32), generator=gen, dtype=torch.float32, device=dev) * 0.2
    drawn = noise.cpu().numpy().copy()
    R = record(A, seeds, steps, interval, G, noise=noise)
    assert R["n_gates"].max() <= G
    written = R["step"] >= 0
    ev = (R["edge_valid"] != 0) & written[:, :, None, None]
    assert not R["noise"][written][R["edge_valid"][written] == 0].any(), "masked cells of a written slot come back 0"
    assert np.array_equal(bits(R["noise"][ev]), bits(drawn[ev])), "evaluated cells come back untouched"
    assert np.array_equal(bits(R["noise"][~written]), bits(drawn[~written])), "unwritten slots are not touched"
    tok = {k: R[k][written] for k in TOK + (("context",) if kind == "context" else ())}
    _, tl = twin.forward_batch(KINDS[kind], w, tok)
    assert np.array_equal(bits(R["logits"][written]), bits(tl)), "the recorded logit is the network's, without the noise"
    clamp = np.float32(w["score_clamp"])
    summed = (R["logits"] + R["noise"]).astype(np.float32)  # ONE float32 addition, exact IEEE on the host
    want = np.tanh(summed.astype(np.float64)) * np.float64(clamp)
    worst = float(np.abs(R["scores"].astype(np.float64) - want)[ev].max())
    bound = 4 * float(np.spacing(clamp))
    print(f"{kind}: max |score - tanh64(f32(logit + noise)) * clamp| = {worst:.3e} (bound {bound:.3e}) over {int(ev.sum())} cells")
    assert worst <= bound
    assert not R["scores"][written][R["edge_valid"][written] == 0].any()
    # the plan: B plans with A's recorded scores of each env's current gate
    per_env = gate_loop(case, n, kind, wname, seeds, interval, True, steps, scores_for=lambda o: R["scores"][np.minimum(o, G - 1), np.arange(n)])
    assert_slots_equal_loop(R, per_env, f"noise {kind}", with_scores=False)
    quiet, _ = _env(case, n, kind, wname)
    Q = record(quiet, seeds, steps, interval, G)

    def trajectory(X, e):  # gate times, plans and S_WPS of env e over its written slots
        wr = X["step"][:, e] >= 0
        return X["step"][:, e].tobytes(), X["selected"][wr, e].tobytes(), X["s_wps_after"][wr, e].tobytes()
    differs = [e for e in range(n) if trajectory(Q, e) != trajectory(R, e)]
    print(f"{kind}: {len(differs)} of {n} trajectories differ from the noise-free run")
    assert len(differs) >= 1, "the noise reached nothing"


# 6. edges (every one deterministic in the inputs chosen, whatever the seed)
def test_edges():
    n, kind, wname = 8, "pair", "init2"
    seeds = np.arange(n, dtype=np.uint64) + 40
    # a gate at step 0, and a gate on the launch's last step: interval 20 and 41 steps -> gates at 0, 20 and 40 = n_steps - 1
    env, w = _env("WPS_hard", n, kind, wname)
    R = record(env, seeds, 41, 20, 41)
    assert (R["step"][0] == 0).all()
    nxt, s_wps = env.tokens("pair", 32, 16), env.metrics()[:, 4]  # the state the launch left: what next_tok of that gate holds
    for e in range(n):
        k = int(R["n_gates"][e]) - 1
        assert R["step"][k, e] == 40, "a gate on the last step"
        for name in TOK:
            assert np.array_equal(bits(R["next_" + name][k, e]), bits(nxt[name][e])), name
        assert R["done"][k, e] == 0 and bits(R["s_wps_after"][k, e]) == bits(s_wps[e])
    # an episode that ends on the step after a gate: max_time_steps = 41, gates at 0, 20, 40; the step after 40 truncates.  60 steps asked for
    p = params_for_case("WPS_hard")
    p.max_time_steps = 41
    env, w = _env("WPS_hard", n, kind, wname, params=p)
    R = record(env, seeds, 60, 20, 60)
    nxt = env.tokens("pair", 32, 16)
    for e in range(n):
        k = int(R["n_gates"][e]) - 1
        assert R["step"][k, e] == 40 and R["done"][k, e] & 2 and (R["done"][:k, e] == 0).all()
        assert (R["step"][k + 1:, e] == -1).all()
        for name in TOK:
            assert np.array_equal(bits(R["next_" + name][k, e]), bits(nxt[name][e])), name
    plain, _ = _env("WPS_hard", n, kind, wname, params=p)
    plain.rollout(seeds, 60, 20, True, True)
    assert_state_equal(state_of(env), state_of(plain), "episode that ends early")
    # gates on consecutive steps: interval 1 -> every step is a gate; next_* of slot k is tok of slot k + 1
    env, w = _env("WPS_hard", n, "context", "init2")
    R = record(env, seeds, 12, 1, 12)
    assert (R["n_gates"] == 12).all() and (R["step"] == np.arange(12)[:, None]).all()
    for name in TOK + ("context",):
        assert np.array_equal(bits(R["next_" + name][:-1]), bits(R[name][1:])), name
    assert np.array_equal(bits(R["s_wps_after"][:-1]), bits(R["s_wps_before"][1:]))


# 7. capacity: at the bound and one past it
@pytest.mark.parametrize("with_noise", [False, True])
def test_capacity(with_noise):
    import torch
    case, n, kind, wname, steps, interval, G = "WPS_hard", 8, "pair", "init2", 100, 20, 3
    seeds = np.arange(n, dtype=np.uint64) + 70
    ample, w = _env(case, n, kind, wname)
    dev = torch.device("cuda", ample.device_index)
    draws = None
    if with_noise:
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        draws = torch.randn((G, n, 16, 32), generator=gen, dtype=torch.float32, device=dev) * 0.2
    # the run with ample slots sees the same draws in its first G slots and none behind them (gates past the capacity are planned without noise)
    big_noise = None
    if with_noise:
        big_noise = torch.zeros((steps, n, 16, 32), dtype=torch.float32, device=dev)
        big_noise[:G] = draws
    W = record(ample, seeds, steps, interval, steps, noise=big_noise)
    assert W["n_gates"].min() > G, "every env has a gate past the capacity"
    env, _ = _env(case, n, kind, wname)
    store = _alloc(env, G + 1, fill=CANARY)
    views = {k: (v if k == "n_gates" else v[:G]) for k, v in store.items()}
    small_noise, nview = None, None
    if with_noise:
        small_noise = torch.full((G + 1, n, 16, 32), float(CANARY), dtype=torch.float32, device=dev)
        small_noise[:G] = draws
        nview = small_noise[:G]
    env.rollout_rl_record(seeds, steps, interval, True, views, noise=nview, write_obs=True)
    env.sync()
    for name, t in store.items():
        a = t.cpu().numpy()
        if name == "n_gates":
            assert np.array_equal(a, W["n_gates"]), "gates are counted past the slots"
            continue
        assert (a[G] == CANARY).all(), f"{name}: slot G was written"
        assert np.array_equal(bits(a[:G]), bits(W[name][:G])), f"{name}: slots below G"
    if with_noise:
        a = small_noise.cpu().numpy()
        assert (a[G] == CANARY).all() and np.array_equal(bits(a[:G]), bits(W["noise"][:G]))
    assert_state_equal(state_of(env), state_of(ample), "capacity: the episode does not depend on the number of slots")
    if not with_noise:
        plain, _ = _env(case, n, kind, wname)
        plain.rollout(seeds, steps, interval, True, True)
        assert_state_equal(state_of(env), state_of(plain), "capacity: against the plain rollout")


# 8. refusals leave the handle usable
def test_refusals_leave_the_handle_usable():
    import torch
    from muavta_amd.batched import BatchedMultiUAVEnv
    case, n = "WPS_hard", 4
    seeds = np.arange(n, dtype=np.uint64)
    env, w = _env(case, n, "pair", "init2")
    dev = torch.device("cuda", env.device_index)
    rings = _alloc(env, 4)

    def call(rl, rec=None, e=env):
        rec = rec or MuavtaRecord()
        if rec.kind == 0 and not rec.task_feats:
            rec.kind = -1
        rec.rl = C.pointer(rl)
        s = np.ascontiguousarray(seeds)
        rc = e.L.muavta_rollout_record(e.h, s.ctypes.data_as(C.c_void_p), 20, 20, 1, 0, C.byref(rec))
        return rc, e.L.muavta_last_error(e.h).decode()

    def full(r=rings, G=4):
        rl = MuavtaRlRings()
        rl.n_slots = G
        for k, t in r.items():
            setattr(rl, k, t.data_ptr())
        return rl

    for G in (0, 4097, -3):
        rc, msg = call(full(G=G))
        assert rc == -1 and "n_slots" in msg
    rl = full()
    rl.selected = None
    rc, msg = call(rl)
    assert rc == -1 and "NULL" in msg
    rl = full()
    rl.context = rings["logits"].data_ptr()
    rc, msg = call(rl)
    assert rc == -1 and "context" in msg
    orings = {k: torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device=dev) for k, (shape, dt) in env.obs_ring_shapes(20).items()}
    rec = MuavtaRecord()
    rec.kind = -1
    for k, t in orings.items():
        setattr(rec, k, t.data_ptr())
    rc, msg = call(full(), rec)
    assert rc == -1 and "observation" in msg
    rec = MuavtaRecord()
    rec.kind, rec.max_tasks, rec.max_agents = 0, 32, 16
    rec.task_feats = rings["logits"].data_ptr()
    rc, msg = call(full(), rec)
    assert rc == -1 and "kind < 0" in msg
    # another mode
    env.set_allocator("hungarian")
    rc, msg = call(full())
    assert rc == -1 and "MUAVTA_ALLOC_MLP_PAIR" in msg
    with pytest.raises(ValueError, match="mlp_pair"):
        env.rollout_rl_record(seeds, 20, 20, True, rings)
    env.set_allocator("mlp_pair")
    # a ContextPair policy without its context rings
    env.set_pair_policy(twin.as_state_dict(twin.load_weights(twin.CONTEXT, "init2")))
    rc, msg = call(full())
    assert rc == -1 and "context" in msg
    with pytest.raises(ValueError, match="context"):
        env.rollout_rl_record(seeds, 20, 20, True, rings)
    # an MLP-Coalition
    env.set_pair_policy(twin.as_checkpoint(twin.load_weights(twin.COALITION, "init2")))
    rc, msg = call(full())
    assert rc == -1 and "MLP-Coalition" in msg
    with pytest.raises(ValueError, match="MLP-Coalition"):
        env.rollout_rl_record(seeds, 20, 20, True, rings)
    env.set_pair_policy(twin.as_state_dict(w))
    # the wide pads (a 24-agent tile takes them)
    wide = BatchedMultiUAVEnv(params_for_case(case, tile_agents=24, tile_tasks=48, tile_threats=24), n)
    wide.set_pair_policy(twin.as_state_dict(w))
    wide.set_allocator("mlp_pair")
    wide.set_token_pads(64, 48)
    rc, msg = call(full(), e=wide)
    assert rc == -1 and "(32, 16)" in msg
    with pytest.raises(ValueError, match=r"\(32, 16\)"):
        wide.rollout_rl_record(seeds, 20, 20, True, rings)
    # what muavta_rollout_record refused before it still refuses, and a record with nothing set is still nothing to record
    with pytest.raises(MuavtaError, match="MLP-Pair"):
        env.rollout_record(seeds, 20, 15, True, obs_rings=orings)
    empty = MuavtaRecord()
    empty.kind = -1
    assert env.L.muavta_rollout_record(env.h, seeds.ctypes.data_as(C.c_void_p), 20, 20, 1, 0, C.byref(empty)) == -1
    # the handle is what it was: a plain rollout gives what a fresh handle gives, and the accepted call works
    env.rollout(seeds, 150, 20, True, True)
    fresh, _ = _env(case, n, "pair", "init2")
    fresh.rollout(seeds, 150, 20, True, True)
    assert_state_equal(state_of(env), state_of(fresh), "after the refusals")
    env.rollout_rl_record(seeds, 150, 20, True, _alloc(env, 64), write_obs=True)
    env.sync()
    assert_state_equal(state_of(env), state_of(fresh), "the accepted call after the refusals")


# 9. lanes
def test_two_lanes_equal_one_lane():
    case, n, kind, wname, steps, interval, G = "WPS_hard_x2", 64, "context", "init2", 150, 20, 32
    sets = [np.arange(k * 1000, k * 1000 + n, dtype=np.uint64) for k in range(2)]
    one, _ = _env(case, n, kind, wname)
    one.set_lanes(1)
    want, want_m = [], []
    for sd in sets:
        want.append(record(one, sd, steps, interval, G))
        want_m.append(one.rollout_metrics())
    two, _ = _env(case, n, kind, wname)
    two.set_lanes(2)
    ring_sets = [_alloc(two, G) for _ in sets]
    for sd, rings in zip(sets, ring_sets):
        two.rollout_rl_record(sd, steps, interval, True, rings, write_obs=True)
    two.sync()
    for k, rings in enumerate(ring_sets):
        for name, t in rings.items():
            a = t.cpu().numpy()
            w_ = want[k][name]
            if name in ("n_gates", "step"):
                assert np.array_equal(a, w_)
                continue
            written = want[k]["step"] >= 0
            assert np.array_equal(bits(a[written]), bits(w_[written])), f"lane set {k}: {name}"
    assert np.array_equal(two.rollout_metrics(back=1), want_m[0]) and np.array_equal(two.rollout_metrics(), want_m[1])


def test_il_rl_record_adds_valid_and_step_reward():
    import torch
    n = 8
    env, w = _env("WPS_hard", n, "pair", "il3")
    seeds = np.arange(n, dtype=np.uint64) + 9
    out = il.rl_record(env, seeds, n_steps=60, interval=20)
    G = 60
    assert out["step"].shape == (G, n) and "noise" not in out
    ng = out["n_gates"].cpu().numpy()
    valid = out["valid"].cpu().numpy()
    assert np.array_equal(valid, np.arange(G)[:, None] < np.minimum(ng, G)[None, :]) and np.array_equal(valid, out["step"].cpu().numpy() >= 0)
    sr = out["step_reward"].cpu().numpy()
    assert np.array_equal(bits(sr[valid]), bits(((out["s_wps_after"].cpu().numpy() - out["s_wps_before"].cpu().numpy()) / 20.0)[valid]))
    gen = torch.Generator(device=torch.device("cuda", env.device_index))
    gen.manual_seed(3)
    noisy = il.rl_record(env, seeds, n_steps=60, interval=20, n_slots=16, noise_std=0.2, generator=gen, rings=None)
    assert noisy["noise"].shape == (16, n, 16, 32) and float(noisy["noise"].abs().max()) > 0
    v = noisy["valid"].cpu().numpy()
    assert not noisy["noise"].cpu().numpy()[v][noisy["edge_valid"].cpu().numpy()[v] == 0].any()
