"""No-GPU checks of the learned MLP-Coalition policy: the fixtures recorded from the reference (tools/gen_golden_mlp_coalition.py) are
consistent and meet the condition the GPU episode test rests on, the host twin of the device's arithmetic (tests/policy_mlp_py.py)
agrees with the reference's float64 evaluation within the bound the GPU test uses, the parser accepts and refuses what the issue lists,
and the frozen C ABI / Python surface carries the new kind without a new symbol or allocator number."""
import glob
import os
import re

import numpy as np
import pytest

import policy_mlp_py as twin
from muavta_amd import native
from muavta_amd.batched import POLICY_KINDS, BatchedMultiUAVEnv
from muavta_amd.native import MuavtaError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TRACES = sorted(glob.glob(os.path.join(GOLDEN, "mlpcoal_trace_*.npz")))
METRICS = sorted(glob.glob(os.path.join(GOLDEN, "mlpcoal_metrics_*.npz")))
KEYS = twin.KEYS


def _weights(name):
    return twin.load_weights(twin.COALITION, name)


def _valid(g):
    return (g["ev"] != 0) & (g["amask"] == 0)[:, :, None] & (g["tmask"] == 0)[:, None, :]


# 1. fixtures
def test_fixture_sets_are_complete_and_meet_the_episode_condition():
    for name in ("init2", "ac3", "wide"):
        w = _weights(name)
        assert w["w0"].shape == (256, 38) and w["b0"].shape == (256,) and w["w1"].shape == (256, 256) and w["w2"].shape == (1, 256) and w["b2"].shape == (1,)
    assert not np.array_equal(_weights("init2")["w1"], _weights("ac3")["w1"])
    assert {(str(g["case"]), str(g["weights"]), int(g["interval"]), int(g["seed"])) for g in map(np.load, TRACES)} == {
        ("WPS_escort", "init2", 12, 0), ("WPS_escort24", "init2", 12, 0), ("WPS_hard", "init2", 12, 0), ("WPS_burst64", "init2", 12, 0), ("WPS_escort", "ac3", 12, 1)}
    for p in TRACES + METRICS + glob.glob(os.path.join(GOLDEN, "mlpcoal_weights_*.npz")):
        assert os.path.getsize(p) < 400 * 1024, p
    # the condition the GPU episode test's cap rests on: E >= 48 over >= 3 cases with F_ref <= E / 10 (weight set init2)
    E = F = 0
    cases = set()
    assert len(METRICS) == 4
    for p in METRICS:
        g = np.load(p)
        n = g["metrics32"].shape[0]
        assert g["metrics64"].shape == (n, 30) and n == (16 if str(g["weights"]) == "init2" else 8) and int(g["interval"]) == 12
        if str(g["weights"]) == "init2":
            differ = [not (np.array_equal(a, b) and ra == rb) for a, b, ra, rb in zip(g["metrics32"], g["metrics64"], g["n_replans32"], g["n_replans64"])]
            E += len(differ); F += sum(differ); cases.add(str(g["case"]))
    assert E >= 48 and len(cases) >= 3 and F * 10 <= E, (E, F, cases)


@pytest.mark.parametrize("path", TRACES, ids=lambda p: os.path.basename(p)[:-4])
def test_trace_is_consistent(path):
    g = np.load(path)
    P = len(g["step"])
    assert P >= 10 and np.array_equal(np.nonzero(g["replanned"])[0], g["step"])
    assert g["tf"].shape == (P, 48, 22) and g["af"].shape == (P, 16, 16) and g["ev"].shape == (P, 16, 48)
    assert g["scores"].dtype == np.float32 and g["logits"].dtype == np.float32 and g["scores64"].dtype == np.float64
    ok = _valid(g)
    assert np.array_equal(ok, g["ev"] != 0)  # edge_valid is 0 on every pad pair (the device masks by edge_valid and by both pad masks)
    for k in range(P):
        assert np.array_equal(g["amask"][k] != 0, g["aid"][k] < 0) and np.array_equal(g["tmask"][k] != 0, g["tid"][k] < 0)
    assert not g["scores"][~ok].any() and not g["scores64"][~ok].any() and not g["logits"][~ok].any()
    assert np.all((g["scores"][ok] > 0) & (g["scores"][ok] < 1))
    assert float(g["d_ref"]) == float(np.abs(g["scores"].astype(np.float64) - g["scores64"])[ok].max()) and 0 < float(g["d_ref"]) < 1e-6
    assert g["selected"].shape == (P, 16, 48) and g["commit_until"].shape[0] == P


# 2. the twin
@pytest.mark.parametrize("path", TRACES, ids=lambda p: os.path.basename(p)[:-4])
def test_twin_vs_reference_float64(path):
    """max |forward32 scores - scores64| over the valid entries <= 4 x D_ref of this trace (the bound of the GPU test), masked cells are 0, and
    forward64 reproduces the fixture's scores64.  Every eighth plan: the twin walks 10 K fma steps per pair in numpy."""
    g = np.load(path)
    w = _weights(str(g["weights"]))
    D = float(g["d_ref"])
    ok = _valid(g)
    worst = 0.0
    for k in range(0, len(g["step"]), 8):
        s, lg = twin.forward(twin.COALITION, w, twin.trace_tokens(g, k))
        assert not s[~ok[k]].any() and not lg[~ok[k]].any()
        worst = max(worst, float(np.abs(s.astype(np.float64) - g["scores64"][k])[ok[k]].max()) if ok[k].any() else 0.0)
        s64, _ = twin.forward64(twin.COALITION, w, twin.trace_tokens(g, k))
        # (the generator wrote scores64 with this very function: the line only catches drift between the twin's file and the fixtures.  The
        # independent link to the reference is torch's own float32 `scores` in the fixture, within d_ref < 1e-6 of scores64 — test_trace_is_consistent.)
        assert np.array_equal(s64, g["scores64"][k])
    print(f"{os.path.basename(path)}: D_ref {D:.3e}, twin {worst:.3e}, ratio {worst / D:.2f}")
    assert worst <= 4 * D


def test_twin_is_a_pure_function_of_the_pair_and_clips_at_20():
    g = np.load(TRACES[0])
    w = _weights("wide")
    k = len(g["step"]) // 2
    af, tf = g["af"][k].copy(), g["tf"][k].copy()
    am, tm = np.zeros(16, np.uint8), np.zeros(48, np.uint8)
    af[5], af[9], tf[7], tf[40] = af[2], af[2], tf[3], tf[3]       # duplicated rows
    ev = np.zeros((16, 48), np.float32); ev[[2, 5, 9]] = 1; ev[:, [3, 7, 40]] = 1
    s, lg = twin.forward(twin.COALITION, w, {"agent_feats": af, "agent_mask": am, "task_feats": tf, "task_mask": tm, "edge_valid": ev})
    u = lg.view(np.uint32)
    assert np.array_equal(u[5], u[2]) and np.array_equal(u[9], u[2]) and np.array_equal(u[:, 7], u[:, 3]) and np.array_equal(u[:, 40], u[:, 3])
    # a plan of the 24-agent escort case with the wide set: both clip sides, each one value — sigmoid at +-20 itself
    g = np.load(os.path.join(GOLDEN, "mlpcoal_trace_WPS_escort24_s0.npz"))
    kk = int(np.nonzero(g["step"] == 40)[0][0])   # a plan whose logits straddle both bounds
    sw, lw = twin.forward(twin.COALITION, w, twin.trace_tokens(g, kk))
    on = g["ev"][kk] != 0
    assert (lw[on] > 20).any() and (lw[on] < -20).any() and (np.abs(lw[on]) < 20).any()
    assert np.all(sw[on & (lw > 20)] == twin.sigmoid32(np.float32(20))) and np.all(sw[on & (lw < -20)] == twin.sigmoid32(np.float32(-20)))
    assert twin.sigmoid32(np.float32(20)) == np.float32(1.0) and 0 < twin.sigmoid32(np.float32(-20)) < 3e-9
    assert np.abs(sw.astype(np.float64) - twin.sigmoid64(lw))[on].max() <= 4 * 2.0 ** -24
    # a pad row masks its pairs whatever edge_valid says
    am[5] = 1
    s2, lg2 = twin.forward(twin.COALITION, w, {"agent_feats": af, "agent_mask": am, "task_feats": tf, "task_mask": tm, "edge_valid": ev})
    assert not s2[5].any() and not lg2[5].any() and np.array_equal(s2[2], s[2])


# 3. the parser
def test_weights_load_through_the_parser():
    for name in ("init2", "ac3", "wide"):
        w = _weights(name)
        sd = twin.as_state_dict(w)
        sd["value_mlp.0.weight"] = np.zeros((256, 48 * 22 + 16 * 16), np.float32)   # the value head is ignored
        sd["value_mlp.2.bias"] = np.zeros(1, np.float32)
        pol = BatchedMultiUAVEnv.parse_pair_policy(sd)
        assert pol["kind"] == "coalition" and pol["hidden"] == 256 and int(pol["raw_features"]) == 2
        for k in KEYS:
            assert pol[k].dtype == np.float32 and pol[k].flags["C_CONTIGUOUS"] and np.array_equal(pol[k], w[k])


def test_parser_reads_a_saved_checkpoint_and_refuses_what_the_device_cannot_run(tmp_path):
    torch = pytest.importorskip("torch")
    w = _weights("init2")
    sd = {k: torch.from_numpy(np.array(v)) for k, v in twin.as_state_dict(w).items()}
    sd["value_mlp.0.weight"] = torch.zeros(256, 48 * 22 + 16 * 16)
    ck = dict(twin.as_checkpoint(w), state_dict=sd)
    path = str(tmp_path / "policy_MLPCoalition.pth")
    torch.save(ck, path)
    for src in (path, ck):
        pol = BatchedMultiUAVEnv.parse_pair_policy(src)
        assert pol["kind"] == "coalition" and pol["hidden"] == 256 and int(pol["raw_features"]) == 2
        assert np.array_equal(pol["w0"], w["w0"]) and np.array_equal(pol["w1"], w["w1"]) and np.array_equal(pol["b2"], w["b2"])

    class Net:
        def state_dict(self):
            return sd

    class Escort:  # what the parser reads of an AttentionEscort: no raw_features attribute
        net, use_attention, commit_threshold, max_tasks, max_agents = Net(), False, 0.5, 48, 16
    assert BatchedMultiUAVEnv.parse_pair_policy(Escort())["kind"] == "coalition"

    class AttEscort(Escort):
        use_attention = True
    with pytest.raises(ValueError, match="Att-Coalition"):
        BatchedMultiUAVEnv.parse_pair_policy(AttEscort())
    with pytest.raises(ValueError, match="Att-Coalition"):
        BatchedMultiUAVEnv.parse_pair_policy(dict(ck, use_attention=True))
    for key, bad in (("version", 1), ("max_tasks", 32), ("max_agents", 24)):
        with pytest.raises(ValueError, match=key):
            BatchedMultiUAVEnv.parse_pair_policy(dict(ck, **{key: bad}))

    class SmallEscort(Escort):
        max_tasks = 32
    with pytest.raises(ValueError, match="max_tasks"):
        BatchedMultiUAVEnv.parse_pair_policy(SmallEscort())
    z = lambda *shape: np.zeros(shape, np.float32)  # noqa: E731
    narrow = {"pair_mlp.0.weight": z(128, 38), "pair_mlp.0.bias": z(128), "pair_mlp.2.weight": z(128, 128), "pair_mlp.2.bias": z(128),
              "pair_mlp.4.weight": z(1, 128), "pair_mlp.4.bias": z(1)}
    with pytest.raises(ValueError, match="hidden = 128"):
        BatchedMultiUAVEnv.parse_pair_policy(narrow)
    with pytest.raises(ValueError, match="hidden = 128"):
        BatchedMultiUAVEnv.parse_pair_policy(dict(ck, state_dict=narrow))
    with pytest.raises(ValueError, match="pair_mlp.0.weight"):   # a 25-column net under an AttentionEscort checkpoint
        BatchedMultiUAVEnv.parse_pair_policy(dict(ck, state_dict=twin.as_state_dict(twin.load_weights(twin.PAIR, "init2"))))
    bad = twin.as_state_dict(w)
    bad["pair_mlp.2.weight"] = z(256, 128)
    with pytest.raises(ValueError, match="pair_mlp.2.weight"):
        BatchedMultiUAVEnv.parse_pair_policy(bad)


def test_every_old_refusal_of_the_parser_still_holds():
    w128, w192 = twin.load_weights(twin.PAIR, "init2"), twin.load_weights(twin.CONTEXT, "init2")
    assert BatchedMultiUAVEnv.parse_pair_policy(twin.as_state_dict(w128))["kind"] == "pair"
    assert BatchedMultiUAVEnv.parse_pair_policy(twin.as_state_dict(w192))["kind"] == "context"
    ck = {"state_dict": {k: v for k, v in twin.as_state_dict(w192).items() if k.startswith("pair_mlp")}, "use_attention": False,
          "max_tasks": 32, "max_agents": 16, "score_clamp": 0.35, "raw_features": False, "kind": "MLPContextPair"}
    with pytest.raises(ValueError, match="Att-ContextPair"):
        BatchedMultiUAVEnv.parse_pair_policy(dict(ck, use_attention=True, kind="AttContextPair"))
    with pytest.raises(ValueError, match="GNN"):
        BatchedMultiUAVEnv.parse_pair_policy(dict(ck, kind="GNNContextPair"))
    with pytest.raises(ValueError, match="use_attention"):
        BatchedMultiUAVEnv.parse_pair_policy(dict(ck, use_attention=True))
    with pytest.raises(ValueError, match="raw_features"):
        BatchedMultiUAVEnv.parse_pair_policy(dict(twin.as_state_dict(w192), raw_features=True))
    with pytest.raises(ValueError, match="pair_mlp.0.weight"):
        BatchedMultiUAVEnv.parse_pair_policy(dict(ck, kind="PairCostHybrid"))
    with pytest.raises(ValueError, match="pair_mlp.0.weight"):   # a 38-column net under a pair / context checkpoint is not a coalition
        BatchedMultiUAVEnv.parse_pair_policy(dict(ck, state_dict=twin.as_state_dict(_weights("init2"))))
    z = lambda *shape: np.zeros(shape, np.float32)  # noqa: E731
    with pytest.raises(ValueError, match="hidden = 64"):
        BatchedMultiUAVEnv.parse_pair_policy({"pair_mlp.0.weight": z(64, 25), "pair_mlp.0.bias": z(64), "pair_mlp.2.weight": z(64, 64), "pair_mlp.2.bias": z(64),
                                              "pair_mlp.4.weight": z(1, 64), "pair_mlp.4.bias": z(1)})
    with pytest.raises(ValueError, match="expected a checkpoint path"):
        BatchedMultiUAVEnv.parse_pair_policy(3)
    with pytest.raises(ValueError, match="no pair_mlp"):
        BatchedMultiUAVEnv.parse_pair_policy({"encoder.0.weight": z(4, 4)})


# 4. the surface
def test_the_frozen_surface_carries_the_new_kind():
    native.build()
    L = native.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "muavta.h")).read(), flags=re.S)
    assert len(native.EXPORTS) == 68 and len(re.findall(r"^\s*(?:int|const char\s*\*)\s+muavta_\w+\s*\(", text, flags=re.M)) == 68
    assert re.search(r"MUAVTA_ALLOC_MLP_PAIR\s*=\s*6\s*\}", text) and re.search(r"MUAVTA_TOK_ESCORT\s*=\s*2\b", text)
    assert BatchedMultiUAVEnv.ALLOCATORS["mlp_coalition"] == 6 == BatchedMultiUAVEnv.ALLOCATORS["mlp_pair"]
    assert max(BatchedMultiUAVEnv.ALLOCATORS.values()) == 6
    assert [f for f, *_ in native.MuavtaPairMlp._fields_] == ["raw_features", "hidden", "score_clamp", "w0", "b0", "w1", "b1", "w2", "b2"]
    assert L.muavta_set_pair_policy(None, None) == -1  # MUAVTA_E_ARG, no device touched
    header = open(os.path.join(ROOT, "include", "muavta.h")).read()
    assert "MLP-Coalition [N, 16, 48]" in header and "score_clamp is IGNORED" in header


def test_set_allocator_kind_names_need_a_policy_of_their_kind():
    env = BatchedMultiUAVEnv.__new__(BatchedMultiUAVEnv)   # no handle: the name is refused before the library is called
    needs = {k.alias: k for k in POLICY_KINDS.values() if k.alias}
    assert {name: k.label for name, k in needs.items()} == {"mlp_context_pair": "MLP-ContextPair", "mlp_coalition": "MLP-Coalition"}
    for name, need in needs.items():
        for rec in [None] + [{"kind": other} for other in POLICY_KINDS if other != need.name]:
            env._pair_policy = rec
            with pytest.raises(MuavtaError, match=need.label):
                env.set_allocator(name)
