"""No-GPU checks of the learned MLP-ContextPair policy: the fixtures recorded from the reference (tools/gen_golden_mlp_context_pair.py)
are consistent and meet the condition the GPU episode test rests on, the host twin of the device's arithmetic
(tests/policy_mlp_py.py) agrees with the reference's float64 evaluation within the bound the GPU test uses, the column
permutation and the pools are what the contract says, and the C ABI / Python surface carries the new entry point."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import policy_mlp_py as twin
from muavta_amd import native
from muavta_amd.batched import BatchedMultiUAVEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TRACES = sorted(glob.glob(os.path.join(GOLDEN, "mlpctx_trace_*.npz")))
WEIGHTS = sorted(glob.glob(os.path.join(GOLDEN, "mlpctx_weights_*.npz")))
METRICS = sorted(glob.glob(os.path.join(GOLDEN, "mlpctx_metrics_*.npz")))
KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")


def _weights(name):
    return twin.load_weights(twin.CONTEXT, name)


# 1. fixtures
def test_fixture_sets_are_complete_and_meet_the_episode_condition():
    assert {os.path.basename(p)[len("mlpctx_weights_"):-4] for p in WEIGHTS} == {"init2", "init2_raw", "il3"}
    assert len(TRACES) == 7 and len(METRICS) == 5
    sets = {name: _weights(name) for name in twin.weight_sets(twin.CONTEXT)}
    for name, w in sets.items():
        assert w["raw_features"] == (name == "init2_raw")
        assert w["w0"].shape == (192, 41 if w["raw_features"] else 58) and w["w1"].shape == (192, 192) and w["w2"].shape == (1, 192)
    assert {(str(g["case"]), str(g["weights"]), int(g["interval"])) for g in map(np.load, TRACES)} == {
        ("WPS_attn", "init2", 15), ("WPS_hard", "init2", 15), ("WPS_hard_x2", "init2", 15), ("WPS_escort24", "init2", 15), ("WPS_burst64", "init2", 15),
        ("WPS_attn", "init2_raw", 20), ("WPS_attn", "il3", 20)}
    for p in TRACES + WEIGHTS + METRICS:
        assert os.path.getsize(p) < 400 * 1024, p
    # the condition the GPU episode test's cap rests on: E >= 48 over >= 3 cases with F_ref <= E / 10 (weight set init2, interval 15)
    E = F = 0
    cases = set()
    for p in METRICS:
        g = np.load(p)
        n = g["metrics32"].shape[0]
        assert g["metrics64"].shape == (n, 30) and n == (16 if str(g["weights"]) == "init2" else 8)
        if str(g["weights"]) == "init2" and int(g["interval"]) == 15:
            differ = [not (np.array_equal(a, b) and ra == rb) for a, b, ra, rb in zip(g["metrics32"], g["metrics64"], g["n_replans32"], g["n_replans64"])]
            E += len(differ); F += sum(differ); cases.add(str(g["case"]))
    assert E >= 48 and len(cases) >= 3 and F * 10 <= E, (E, F, cases)


@pytest.mark.parametrize("path", TRACES, ids=lambda p: os.path.basename(p)[:-4])
def test_trace_is_consistent(path):
    g = np.load(path)
    w = _weights(str(g["weights"]))
    P = len(g["step"])
    da, dt, c = twin.dims(w["raw_features"])
    assert P >= 10 and np.array_equal(np.nonzero(g["replanned"])[0], g["step"])
    assert g["tf"].shape == (P, 32, dt) and g["af"].shape == (P, 16, da) and g["ev"].shape == (P, 16, 32) and g["ctx"].shape == (P, c)
    assert g["ctx"].dtype == np.float32 and g["scores"].dtype == np.float32 and g["scores64"].dtype == np.float64
    assert g["tmask"].shape == (P, 32) and g["amask"].shape == (P, 16)
    for k in range(P):
        assert np.array_equal(g["amask"][k] != 0, g["aid"][k] < 0) and np.array_equal(g["tmask"][k] != 0, g["tid"][k] < 0)
        assert not g["scores"][k][g["ev"][k] == 0].any() and not g["scores64"][k][g["ev"][k] == 0].any()
    ev = g["ev"] != 0
    assert float(g["d_ref"]) == float(np.abs(g["scores"].astype(np.float64) - g["scores64"])[ev].max()) and 0 < float(g["d_ref"]) < 1e-6


# 2. the twin
@pytest.mark.parametrize("path", TRACES, ids=lambda p: os.path.basename(p)[:-4])
def test_twin_vs_reference_float64(path):
    """max |twin scores - scores64| over the valid entries <= 4 x D_ref of this trace (the bound of the GPU test), and forward64
    reproduces the fixture's scores64.  Every third plan: the twin walks 442 fma steps per pair in numpy."""
    g = np.load(path)
    w = _weights(str(g["weights"]))
    D = float(g["d_ref"])
    worst = 0.0
    for k in range(0, len(g["step"]), 3):
        s, lg = twin.forward(twin.CONTEXT, w, twin.trace_tokens(g, k))
        ev = g["ev"][k] != 0
        assert not s[~ev].any() and not lg[~ev].any()
        worst = max(worst, float(np.abs(s.astype(np.float64) - g["scores64"][k])[ev].max()) if ev.any() else 0.0)
        s64, _ = twin.forward64(twin.CONTEXT, w, twin.trace_tokens(g, k))
        # (the generator wrote scores64 with this very function: the line only catches drift between the twin's file and the fixtures.  The
        # independent link to the reference is torch's own float32 `scores` in the fixture, within d_ref < 1e-6 of scores64 — test_trace_is_consistent.)
        assert np.array_equal(s64, g["scores64"][k])
    print(f"{os.path.basename(path)}: D_ref {D:.3e}, twin {worst:.3e}, ratio {worst / D:.2f}")
    assert worst <= 4 * D


@pytest.mark.parametrize("raw", [False, True])
def test_column_permutation(raw):
    """device order = a_pool, t_pool, context, agent, task; state_dict order = agent, task, a_pool, t_pool, context.  With weights that
    pick out ONE input column each, layer 1's outputs name the input each device position reads."""
    da, dt, c = twin.dims(raw)
    K = 2 * (da + dt) + c
    perm = twin.device_columns(raw)
    assert sorted(perm.tolist()) == list(range(K))
    names = [("agent", d) for d in range(da)] + [("task", d) for d in range(dt)] + [("a_pool", d) for d in range(da)] + [("t_pool", d) for d in range(dt)] + \
            [("ctx", d) for d in range(c)]
    want = [("a_pool", d) for d in range(da)] + [("t_pool", d) for d in range(dt)] + [("ctx", d) for d in range(c)] + [("agent", d) for d in range(da)] + \
           [("task", d) for d in range(dt)]
    assert [names[p] for p in perm] == want
    # through the twin: an identity layer 1 in state_dict order applied to a device-order row gives the row back in state_dict order
    w = {"w0": np.eye(192, K, dtype=np.float32), "b0": np.zeros(192, np.float32)}
    x = (np.arange(K, dtype=np.float32) + 1)[None, :]            # device-order row: position k holds k + 1
    h = twin.linear(np.ascontiguousarray(w["w0"][:, perm]), w["b0"], x)[0, :K]
    assert np.array_equal(h, (np.argsort(perm) + 1).astype(np.float32))


def test_pools():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((16, 12)).astype(np.float32)
    # count 0: every row a pad -> 0 / max(0, 1) = +0.0 in every column
    p = twin.pool(x, np.ones(16, np.uint8))
    assert np.array_equal(p.view(np.uint32), np.zeros(12, np.float32).view(np.uint32))
    # one row: 0.0f + x, divided by 1: the row itself (and -0.0 becomes +0.0: the sum starts from +0.0)
    m = np.ones(16, np.uint8); m[5] = 0
    x[5, 0] = np.float32(-0.0)
    p = twin.pool(x, m)
    assert np.array_equal(p[1:], x[5, 1:]) and p[0].view(np.uint32) == 0
    # a pad row in the middle is skipped, the others are added in ascending order, one rounding per add, one division
    m = np.zeros(16, np.uint8); m[7] = 1
    s = np.zeros(12, np.float32)
    for r in range(16):
        if r != 7:
            s = (s + x[r]).astype(np.float32)
    assert np.array_equal(twin.pool(x, m).view(np.uint32), (s / np.float32(15)).astype(np.float32).view(np.uint32))
    # ... and the order matters at float32: the descending sum differs somewhere for this data, so an ascending-order twin pins the order
    big = (rng.standard_normal((32, 13)) * rng.choice([1e-3, 1.0, 1e3], (32, 1))).astype(np.float32)
    s_desc = np.zeros(13, np.float32)
    for r in range(31, -1, -1):
        s_desc = (s_desc + big[r]).astype(np.float32)
    assert not np.array_equal(twin.pool(big, np.zeros(32, np.uint8)), (s_desc / np.float32(32)).astype(np.float32))
    # the float64 yardstick pools the same rows
    g = np.load(TRACES[0])
    w = _weights(str(g["weights"]))
    k = len(g["step"]) // 2
    pre = twin.prefix(g["af"][k], g["amask"][k], g["tf"][k], g["tmask"][k], g["ctx"][k])
    live = g["amask"][k] == 0
    assert 0 < live.sum() and np.allclose(pre[:12], g["af"][k][live].astype(np.float64).mean(0), rtol=1e-6, atol=1e-7) and np.array_equal(pre[25:], g["ctx"][k])


def test_twin_is_a_pure_function_of_the_pair_within_an_env():
    g = np.load(TRACES[0])
    w = _weights(str(g["weights"]))
    k = len(g["step"]) // 2
    af, tf = g["af"][k].copy(), g["tf"][k].copy()
    am, tm = np.zeros(16, np.uint8), np.zeros(32, np.uint8)
    af[5], af[9], tf[7], tf[30] = af[2], af[2], tf[3], tf[3]       # duplicated rows
    ev = np.zeros((16, 32), np.float32); ev[[2, 5, 9]] = 1; ev[:, [3, 7, 30]] = 1
    _, lg = twin.forward(twin.CONTEXT, w, {"agent_feats": af, "agent_mask": am, "task_feats": tf, "task_mask": tm, "context": g["ctx"][k], "edge_valid": ev})
    lg = lg.view(np.uint32)
    assert np.array_equal(lg[5], lg[2]) and np.array_equal(lg[9], lg[2]) and np.array_equal(lg[:, 7], lg[:, 3]) and np.array_equal(lg[:, 30], lg[:, 3])


# 3. the parser
@pytest.mark.parametrize("path", WEIGHTS, ids=lambda p: os.path.basename(p)[:-4])
def test_weights_load_through_the_parser(path):
    w = _weights(os.path.basename(path)[len("mlpctx_weights_"):-4])
    pol = BatchedMultiUAVEnv.parse_pair_policy(twin.as_state_dict(w))
    assert pol["kind"] == "context" and pol["hidden"] == 192 and pol["raw_features"] == w["raw_features"] and pol["score_clamp"] == w["score_clamp"]
    for k in KEYS:
        assert pol[k].dtype == np.float32 and pol[k].flags["C_CONTIGUOUS"] and np.array_equal(pol[k], w[k])
    sd = {k: v for k, v in twin.as_state_dict(w).items() if k.startswith("pair_mlp")}
    sd["ctx_mlp.0.weight"] = np.zeros((192, 33), np.float32)      # value-head entries are ignored
    sd["value_mlp.2.bias"] = np.zeros(1, np.float32)
    pol = BatchedMultiUAVEnv.parse_pair_policy(sd)
    assert pol["kind"] == "context" and pol["raw_features"] == w["raw_features"] and pol["score_clamp"] == 0.35
    assert BatchedMultiUAVEnv.parse_pair_policy(sd, score_clamp=0.2)["score_clamp"] == 0.2


def test_parser_reads_a_saved_checkpoint_and_refuses_what_the_device_cannot_run(tmp_path):
    torch = pytest.importorskip("torch")
    w = _weights("init2")
    sd = {k: torch.from_numpy(np.array(v)) for k, v in twin.as_state_dict(w).items() if k.startswith("pair_mlp")}
    sd["ctx_mlp.0.weight"] = torch.zeros(192, 33)
    sd["value_mlp.0.weight"] = torch.zeros(96, 192)
    ck = {"state_dict": sd, "use_attention": False, "max_tasks": 32, "max_agents": 16, "d_model": 64, "nhead": 4, "n_layers": 2, "lr": 3e-4,
          "score_clamp": 0.35, "raw_features": False, "kind": "MLPContextPair"}
    path = str(tmp_path / "context_pair_mlp.pth")
    torch.save(ck, path)
    for src in (path, ck):
        pol = BatchedMultiUAVEnv.parse_pair_policy(src)
        assert pol["kind"] == "context" and pol["hidden"] == 192 and np.array_equal(pol["w0"], w["w0"]) and np.array_equal(pol["w1"], w["w1"])
        assert pol["score_clamp"] == 0.35 and not pol["raw_features"]

    class Net:
        def state_dict(self):
            return sd

    class Hybrid:  # what the parser reads of a ContextPairHybrid
        net, use_attention, raw_features, score_clamp, kind = Net(), False, False, 0.35, "MLPContextPair"
    assert BatchedMultiUAVEnv.parse_pair_policy(Hybrid())["kind"] == "context"
    # an MLP-Pair still parses as before
    w128 = twin.load_weights(twin.PAIR, "init2")
    pol = BatchedMultiUAVEnv.parse_pair_policy(twin.as_state_dict(w128))
    assert pol["kind"] == "pair" and pol["hidden"] == 128
    # refusals
    with pytest.raises(ValueError, match="Att-ContextPair"):
        BatchedMultiUAVEnv.parse_pair_policy(dict(ck, use_attention=True, kind="AttContextPair"))
    with pytest.raises(ValueError, match="GNN"):
        BatchedMultiUAVEnv.parse_pair_policy(dict(ck, kind="GNNContextPair"))
    with pytest.raises(ValueError, match="use_attention"):
        BatchedMultiUAVEnv.parse_pair_policy(dict(ck, use_attention=True))
    bad = twin.as_state_dict(w)
    bad["pair_mlp.2.weight"] = np.zeros((192, 128), np.float32)
    with pytest.raises(ValueError, match="pair_mlp.2.weight"):
        BatchedMultiUAVEnv.parse_pair_policy(bad)
    with pytest.raises(ValueError, match="raw_features"):
        BatchedMultiUAVEnv.parse_pair_policy(dict(twin.as_state_dict(w), raw_features=True))      # 58 columns are not a raw net
    z = lambda *shape: np.zeros(shape, np.float32)  # noqa: E731
    narrow = {"pair_mlp.0.weight": z(128, 58), "pair_mlp.0.bias": z(128), "pair_mlp.2.weight": z(128, 128), "pair_mlp.2.bias": z(128),
              "pair_mlp.4.weight": z(1, 128), "pair_mlp.4.bias": z(1)}
    with pytest.raises(ValueError, match="hidden = 128"):
        BatchedMultiUAVEnv.parse_pair_policy(narrow)
    with pytest.raises(ValueError, match="pair_mlp.0.weight"):                                    # a 58-column net under an MLP-Pair checkpoint
        BatchedMultiUAVEnv.parse_pair_policy(dict(ck, kind="PairCostHybrid"))


# 4. ABI
NEW = "muavta_set_context_pair_policy"


def test_new_symbol_is_declared_exported_and_bound():
    native.build()
    L = native.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "muavta.h")).read(), flags=re.S)
    assert re.search(rf"^\s*int\s+{NEW}\s*\(", text, flags=re.M), f"{NEW} not declared in include/muavta.h"
    assert hasattr(L, NEW) and NEW in native.EXPORTS and len(native.EXPORTS) == 68
    assert len(re.findall(r"^\s*(?:int|const char\s*\*)\s+muavta_\w+\s*\(", text, flags=re.M)) == 68
    assert L.muavta_set_context_pair_policy(None, None) == -1  # MUAVTA_E_ARG, no device touched
    # no allocator number of its own: mode 6 runs the installed learned pair policy, 7 stays unknown
    assert re.search(r"MUAVTA_ALLOC_MLP_PAIR\s*=\s*6\s*\}", text)
    assert BatchedMultiUAVEnv.ALLOCATORS["mlp_context_pair"] == 6 == BatchedMultiUAVEnv.ALLOCATORS["mlp_pair"]
    assert max(BatchedMultiUAVEnv.ALLOCATORS.values()) == 6 and 7 not in BatchedMultiUAVEnv.ALLOCATORS.values()


def test_context_pair_mlp_struct_matches_the_header(tmp_path):
    st = native.MuavtaContextPairMlp
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "muavta.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(MuavtaContextPairMlp));']
    lines += [f'  printf("{f} %zu\\n", offsetof(MuavtaContextPairMlp, {f}));' for f, *_ in st._fields_] + ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(st)
    for f, *_ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f
