"""No-GPU checks of the learned modes' host reference (tests/learned_lockstep.py): its table of planners replays every episode the reference
recorded under MLP-Pair, MLP-ContextPair and MLP-Coalition on the oracle alone, and the cases of tests/golden/learned_fuzz_cases.json
(tools/find_learned_fuzz_cases.py) are what the oracle and the twin give and cover what the GPU module is meant to meet."""
import glob
import json
import os
import sys

import numpy as np
import pytest

import learned_lockstep as LL
import orc
import policy_mlp_py as twin
import wide_pads as WP
from capacity_cases import TILES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tools"))

TRACES = [(kind, p) for kind, prefix in (("pair", "mlppair_"), ("context", "mlpctx_"), ("coalition", "mlpcoal_"))
          for p in sorted(glob.glob(os.path.join(GOLDEN, prefix + "trace_*.npz")))] + list(WP.ALL_LEARNED_TRACES)


# a. the mapping table is the reference's planner
def replay(kind, g):
    """The episode of a trace fixture on the oracle alone, through LL.TABLE's planner fed the fixture's float32 scores -> plans replayed"""
    w = LL.weights(kind, str(g["weights"]))
    interval, pads = int(g["interval"]), ((int(g["max_tasks"]), int(g["max_agents"])) if "max_tasks" in g else None)
    mt, ma = LL.TABLE[kind].pads(pads)
    o = orc.OracleEnv(WP.params_of(g))
    o.reset(int(g["seed"]))
    steps, k = g["step"].tolist(), 0
    names = {"task_feats": "tf", "agent_feats": "af", "edge_valid": "ev", "task_ids": "tid", "agent_ids": "aid", "task_mask": "tmask", "agent_mask": "amask", "context": "ctx"}
    for t in range(len(g["replanned"])):
        planned = bool(g["replanned"][t])
        if planned:
            assert t == steps[k]
            tok = LL.oracle_tokens(o, kind, w, pads)
            for name, short in names.items():
                if short in g and name in tok:
                    assert np.array_equal(tok[name], g[short][k]), f"t={t}: {name}"
        sc = g["scores"][k] if planned else np.zeros((ma, mt), np.float32)
        aa, ai, sel, replanned = LL.oracle_plan(o, kind, w, interval, True, sc, pads)
        assert replanned == planned, f"t={t}: gate"
        if planned:
            assert np.array_equal(sel, g["selected"][k]), f"t={t}: selected mask"
            if "commit_until" in g:
                assert np.array_equal(o.agent_commit_until(), g["commit_until"][k]), f"t={t}: commit locks"
            k += 1
        else:
            assert len(aa) == 0 and not sel.any()
        o.step(aa, ai)
    assert k == len(steps)
    assert np.array_equal(o.metrics(), g["metrics"]), "final metrics"
    assert o.dims()["n_replans"] == int(g["n_replans"])
    return k


@pytest.mark.parametrize("kind,path", TRACES, ids=[os.path.basename(p)[:-4] for _, p in TRACES])
def test_table_replays_the_reference_trace(kind, path):
    """Every mlppair_ / mlpctx_ / mlpcoal_ trace and the wide-pad ones of tests/wide_pads.py: at each recorded plan the oracle's tokens equal
    the fixture's, the table's planner fed the fixture's scores gives its selected mask and gate bit (MLP-Coalition: its commit locks), and
    the episode ends in the fixture's metrics and n_replans.  What a fixture lacks is not compared: the MLP-Pair traces hold no pad masks
    (tmask / amask) and no trace of the pair kinds holds commit locks; the token ids (tid / aid), which every trace holds, are compared."""
    g = np.load(path)
    assert replay(kind, g) == len(g["step"]) >= 10


def test_table_takes_its_numbers_from_the_scored_fuzz_leg():
    from fuzz_device import SCORED
    from test_gpu_parity import GATE
    for kind, P in LL.TABLE.items():
        gate, flags = P.gate_flags
        assert gate == GATE[P.gate] and (P.gate, dict(P.kw), flags) in [(r[0], r[1], r[4]) for r in SCORED]
    assert LL.TABLE["pair"].gate_flags == LL.TABLE["context"].gate_flags == (GATE["trainer"], 1) and LL.TABLE["coalition"].gate_flags == (GATE["escort"], 4)
    for kind, names in LL.WEIGHT_SETS.items():
        assert set(names) == set(twin.weight_sets(LL.TABLE[kind].twin))


# b. case selection
def cases():
    with open(os.path.join(GOLDEN, "learned_fuzz_cases.json")) as f:
        return json.load(f)["cases"]


def test_selection_has_the_sizes_and_stays_below_every_tile_bound():
    import find_learned_fuzz_cases as F
    cs = cases()
    assert len({c["id"] for c in cs}) == len(cs)
    for kind in LL.TABLE:
        narrow = [c for c in cs if c["kind"] == kind and tuple(c["pads"]) == LL.TABLE[kind].pads()]
        assert len(narrow) == 12 and {c["tile"][0] for c in narrow} == {16, 24, 64}, kind
        assert {c["weights"] for c in cs if c["kind"] == kind} == set(LL.WEIGHT_SETS[kind]), kind
    wide = [c for c in cs if tuple(c["pads"]) == LL.WIDE]
    assert len(wide) == 6 and {c["tile"][0] for c in wide} == {24, 64} and {c["kind"] for c in wide} == {"pair", "context"}
    assert len(cs) == 42
    for c in cs:
        assert len(c["seeds"]) == 3 and c["steps"] <= 260 and len(c["gates"]) == 3
        tl = TILES[c["tile"][0]]
        for peaks in c["peaks"]:
            assert not LL.fits(tl, peaks, margin=F.MARGIN), (c["id"], peaks)
        cfg = F.wide_config(c["k"])["cfg"]
        assert sum(cfg["agents"].values()) <= tl.A and sum(n for _, n in cfg["threats_list"]) <= tl.H


def test_selection_covers_the_listed_properties():
    import find_learned_fuzz_cases as F
    have = F.coverage(cases())
    missing = [name for name in F.PROPERTIES if not have.get(name)]
    assert not missing, missing
    assert set(F.NOT_FOUND) <= set(F.PROPERTIES_ASKED) and set(F.PROPERTIES) | set(F.NOT_FOUND) == set(F.PROPERTIES_ASKED)


@pytest.mark.parametrize("which", ["pair-init2-t16-32x16-small1", "coalition-ac3-t16-48x16-small2001", "context-init2-t24-64x48-small1000"])
def test_entry_is_what_the_oracle_and_the_twin_give(which):
    """three entries of the file (one per kind; the last a wide-pad one) derived again from the oracle and the twin"""
    import find_learned_fuzz_cases as F
    c = next(c for c in cases() if c["id"] == which)
    again = F.entry(c["k"], tuple(c["tile"]), c["kind"], c["weights"], tuple(c["pads"]))
    for key in ("seeds", "interval", "use_vis", "steps", "gates", "n_replans", "peaks", "props"):
        assert again[key] == c[key], (c["id"], key)
