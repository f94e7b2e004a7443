"""No-GPU checks of the learned MLP-Pair mode: the fixtures recorded from the reference (tools/gen_golden_mlp_pair.py) are consistent,
the host twin of the device's arithmetic (tests/policy_mlp_py.py) agrees with the reference's float64 evaluation within the bound the GPU
test uses, and the C ABI / Python surface carries the new entry points."""
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
TRACES = sorted(glob.glob(os.path.join(GOLDEN, "mlppair_trace_*.npz")))
WEIGHTS = sorted(glob.glob(os.path.join(GOLDEN, "mlppair_weights_*.npz")))
METRICS = sorted(glob.glob(os.path.join(GOLDEN, "mlppair_metrics_*.npz")))


def _weights(name):
    return twin.load_weights(twin.PAIR, name)


def d_ref(g):
    """the reference's own float32 deviation from a float64 evaluation of the same net on the same tokens"""
    ev = g["ev"] != 0
    return float(np.abs(g["scores"].astype(np.float64) - g["scores64"])[ev].max())


# 1. fixture integrity
def test_fixture_sets_are_complete():
    assert len(WEIGHTS) >= 3 and len(TRACES) >= 6 and len(METRICS) >= 4
    sets = {name: _weights(name) for name in twin.weight_sets(twin.PAIR)}
    assert any(w["raw_features"] for w in sets.values()) and any(not w["raw_features"] for w in sets.values())
    for p in TRACES + METRICS:
        assert str(np.load(p)["weights"]) in sets, p
    for p in TRACES + WEIGHTS + METRICS:
        assert os.path.getsize(p) < 400 * 1024, p
    # the condition the GPU episode test's cap rests on: E >= 48 over >= 3 cases with F_ref <= E / 10 (weight set init2, interval 15)
    E = F = 0
    cases = set()
    for p in METRICS:
        g = np.load(p)
        if str(g["weights"]) == "init2" and int(g["interval"]) == 15:
            differ = [not (np.array_equal(a, b) and ra == rb) for a, b, ra, rb in zip(g["metrics32"], g["metrics64"], g["n_replans32"], g["n_replans64"])]
            E += len(differ); F += sum(differ); cases.add(str(g["case"]))
    assert E >= 48 and len(cases) >= 3 and F * 10 <= E, (E, F, cases)


@pytest.mark.parametrize("path", TRACES, ids=lambda p: os.path.basename(p)[:-4])
def test_trace_is_consistent(path):
    g = np.load(path)
    w = _weights(str(g["weights"]))
    P = len(g["step"])
    assert P >= 10 and P == int(g["replanned"].sum()) and np.array_equal(np.nonzero(g["replanned"])[0], g["step"])
    da, dt = (11, 9) if w["raw_features"] else (12, 13)
    assert g["tf"].shape == (P, 32, dt) and g["af"].shape == (P, 16, da) and g["ev"].shape == (P, 16, 32)
    assert g["scores"].dtype == np.float32 and g["logits"].dtype == np.float32 and g["scores64"].dtype == np.float64
    assert int(g["policy_n_replans"]) <= int(g["n_replans"]) <= P
    for k in range(P):
        t, ev, sel = int(g["step"][k]), g["ev"][k], g["selected"][k]
        # edge_valid lives on live rows x kept columns; the scores are masked by it
        assert not ev[g["aid"][k] < 0].any() and not ev[:, g["tid"][k] < 0].any()
        assert not g["scores"][k][ev == 0].any() and not g["scores64"][k][ev == 0].any()
        # _selected_mask: one cell per result pair whose agent and task are token rows / columns; at most one per row
        pairs = g["pairs"][g["pairs"][:, 0] == t][:, 1:]
        want = np.zeros((16, 32), np.float32)
        for a, tid in pairs:
            i, j = np.nonzero(g["aid"][k] == a)[0], np.nonzero(g["tid"][k] == tid)[0]
            if len(i) and len(j):
                want[i[0], j[0]] = 1
        assert np.array_equal(sel, want), f"plan {k} (t={t})"
        assert sel.sum(axis=1).max() <= 1
        acts = g["actions"][g["actions"][:, 0] == t]
        assert len(acts) <= len(pairs) and set(acts[:, 1].tolist()) <= set(pairs[:, 0].tolist())
    assert g["metrics"].shape == (30,)


@pytest.mark.parametrize("path", WEIGHTS, ids=lambda p: os.path.basename(p)[:-4])
def test_weights_load_through_the_parser(path):
    w = _weights(os.path.basename(path)[len("mlppair_weights_"):-4])
    pol = BatchedMultiUAVEnv.parse_pair_policy(twin.as_state_dict(w))
    assert pol["hidden"] == 128 and pol["raw_features"] == w["raw_features"] and pol["score_clamp"] == w["score_clamp"]
    for k in ("w0", "b0", "w1", "b1", "w2", "b2"):
        assert pol[k].dtype == np.float32 and pol[k].flags["C_CONTIGUOUS"] and np.array_equal(pol[k], w[k])
    assert pol["w0"].shape == (128, 20 if w["raw_features"] else 25)
    # raw_features follows from layer 1's width when the mapping does not say; score_clamp defaults to the reference's SCORE_CLAMP
    sd = {k: v for k, v in twin.as_state_dict(w).items() if k.startswith("pair_mlp")}
    pol = BatchedMultiUAVEnv.parse_pair_policy(sd)
    assert pol["raw_features"] == w["raw_features"] and pol["score_clamp"] == 0.35
    assert BatchedMultiUAVEnv.parse_pair_policy(sd, score_clamp=0.2)["score_clamp"] == 0.2


def test_parser_reads_a_saved_checkpoint_and_refuses_what_the_device_cannot_run(tmp_path):
    torch = pytest.importorskip("torch")
    w = _weights("init2")
    sd = {k: torch.from_numpy(np.array(v)) for k, v in twin.as_state_dict(w).items() if k.startswith("pair_mlp")}
    sd["value_mlp.0.weight"] = torch.zeros(128, 25)
    ck = {"state_dict": sd, "use_attention": False, "max_tasks": 32, "max_agents": 16, "score_clamp": 0.35, "raw_features": False, "kind": "PairCostHybrid"}
    path = str(tmp_path / "pair_cost_mlp.pth")
    torch.save(ck, path)
    pol = BatchedMultiUAVEnv.parse_pair_policy(path)
    assert np.array_equal(pol["w1"], w["w1"]) and pol["score_clamp"] == 0.35 and not pol["raw_features"]
    with pytest.raises(ValueError, match="use_attention"):
        BatchedMultiUAVEnv.parse_pair_policy(dict(ck, use_attention=True))
    with pytest.raises(ValueError, match="pair_mlp"):
        BatchedMultiUAVEnv.parse_pair_policy({"encoder.layers.0.weight": np.zeros(3)})
    bad = twin.as_state_dict(w)
    bad["pair_mlp.2.weight"] = np.zeros((128, 64), np.float32)
    with pytest.raises(ValueError, match="pair_mlp.2.weight"):
        BatchedMultiUAVEnv.parse_pair_policy(bad)
    small = {"pair_mlp.0.weight": np.zeros((64, 25), np.float32), "pair_mlp.0.bias": np.zeros(64, np.float32), "pair_mlp.2.weight": np.zeros((64, 64), np.float32),
             "pair_mlp.2.bias": np.zeros(64, np.float32), "pair_mlp.4.weight": np.zeros((1, 64), np.float32), "pair_mlp.4.bias": np.zeros(1, np.float32)}
    with pytest.raises(ValueError, match="hidden"):
        BatchedMultiUAVEnv.parse_pair_policy(small)
    with pytest.raises(ValueError, match="raw_features"):
        BatchedMultiUAVEnv.parse_pair_policy(dict(twin.as_state_dict(w), raw_features=True))
    with pytest.raises(ValueError):
        BatchedMultiUAVEnv.parse_pair_policy(3)


# 2. host twin vs fixture
def test_fma32_is_correctly_rounded():
    from fractions import Fraction
    rng = np.random.default_rng(0)
    n = 3000
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    c = (rng.standard_normal(n) * rng.choice([1e-6, 1.0, 1e3], n)).astype(np.float32)
    # products that land exactly half way between two float32 neighbours, nudged by an addend far below the last bit
    h = np.float32(1 + 2.0 ** -12)
    a = np.concatenate([a, [h, h, h]]).astype(np.float32); b = np.concatenate([b, [h, h, h]]).astype(np.float32)
    c = np.concatenate([c, [0.0, 1e-30, -1e-30]]).astype(np.float32)
    got = twin.fma32(a, b, c)
    for i in range(len(a)):
        v = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        f = np.float32(float(v))
        cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
        best = min(cands, key=lambda x: (abs(Fraction(float(x)) - v), int(np.float32(x).view(np.uint32)) & 1))
        assert got[i].view(np.uint32) == np.float32(best).view(np.uint32), (a[i], b[i], c[i])
    assert float(got[-2]) > float(got[-3]) == float(got[-1])


@pytest.mark.parametrize("path", TRACES, ids=lambda p: os.path.basename(p)[:-4])
def test_twin_vs_reference_float64(path):
    """max |twin scores - scores64| over the valid entries <= 4 x D_ref, D_ref = the reference's own max |scores - scores64| on this
    trace: the bound of the GPU test (a k-ordered float32 chain deviates about as much as torch's own float32 order does)."""
    g = np.load(path)
    w = _weights(str(g["weights"]))
    D = d_ref(g)
    assert 0 < D < 1e-6
    worst = 0.0
    for k in range(len(g["step"])):
        s, lg = twin.forward(twin.PAIR, w, twin.trace_tokens(g, k))
        ev = g["ev"][k] != 0
        assert not s[~ev].any() and not lg[~ev].any()
        worst = max(worst, float(np.abs(s.astype(np.float64) - g["scores64"][k])[ev].max()) if ev.any() else 0.0)
        s64, _ = twin.forward64(twin.PAIR, w, twin.trace_tokens(g, k))
        assert np.array_equal(s64, g["scores64"][k])
    print(f"{os.path.basename(path)}: D_ref {D:.3e}, twin {worst:.3e}, ratio {worst / D:.2f}")
    assert worst <= 4 * D


def test_twin_is_a_pure_function_of_the_pair():
    g = np.load(TRACES[0])
    w = _weights(str(g["weights"]))
    k = len(g["step"]) // 2
    af, tf = g["af"][k].copy(), g["tf"][k].copy()
    ev = np.ones((16, 32), np.float32)
    af[5], af[9], tf[7], tf[30] = af[2], af[2], tf[3], tf[3]       # duplicated rows
    _, lg = twin.forward(twin.PAIR, w, {"agent_feats": af, "task_feats": tf, "edge_valid": ev})
    assert np.array_equal(lg[5].view(np.uint32), lg[2].view(np.uint32)) and np.array_equal(lg[9].view(np.uint32), lg[2].view(np.uint32))
    assert np.array_equal(lg[:, 7].view(np.uint32), lg[:, 3].view(np.uint32)) and np.array_equal(lg[:, 30].view(np.uint32), lg[:, 3].view(np.uint32))
    rng = np.random.default_rng(1)
    pa, pt = rng.permutation(16), rng.permutation(32)                 # permuted rows / columns, and a sparser mask
    ev2 = (rng.uniform(size=(16, 32)) < 0.3).astype(np.float32)
    _, lg2 = twin.forward(twin.PAIR, w, {"agent_feats": af[pa], "task_feats": tf[pt], "edge_valid": ev2})
    want = np.where(ev2 != 0, lg[pa][:, pt], np.float32(0))
    assert np.array_equal(lg2.view(np.uint32), want.view(np.uint32))


# 3. ABI
NEW = ("muavta_set_pair_policy", "muavta_pair_scores", "muavta_pair_scores_device")


def test_new_symbols_are_declared_exported_and_bound():
    native.build()
    L = native.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "muavta.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"^\s*int\s+{name}\s*\(", text, flags=re.M), f"{name} not declared in include/muavta.h"
        assert hasattr(L, name) and name in native.EXPORTS
    assert re.search(r"MUAVTA_ALLOC_MLP_PAIR\s*=\s*6\b", text)
    assert BatchedMultiUAVEnv.ALLOCATORS["mlp_pair"] == 6
    assert L.muavta_set_pair_policy(None, None) == -1 and L.muavta_pair_scores(None, None, None) == -1  # MUAVTA_E_ARG, no device touched


def test_pair_mlp_struct_matches_the_header(tmp_path):
    st = native.MuavtaPairMlp
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "muavta.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(MuavtaPairMlp));']
    lines += [f'  printf("{f} %zu\\n", offsetof(MuavtaPairMlp, {f}));' for f, *_ in st._fields_] + ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(st)
    for f, *_ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f
