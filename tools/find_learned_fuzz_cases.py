#!/usr/bin/env python3
"""Select the random configurations of tests/test_gpu_learned_fuzz.py and write tests/golden/learned_fuzz_cases.json (data only).  Uses the
oracle and the host twin, no device:

    python tools/find_learned_fuzz_cases.py [--check]

`SLOTS` lists what the selection is made of: 12 cases per learned kind at its default token pads (four on each tile) and 6 at the wide pads
(64, 48), each with a family of tests/fuzz_reference.py::wide_config to draw from (small from k = 0, large from BIG, EDGE from EDGE), a
fleet size, a weight set and the properties the case has to show.  For a slot the ids of its family are scanned in ascending order from
the kind's offset (at most SCAN = 3,000 of them) and the first id is taken

  - whose configuration has the slot's properties that can be read off it, and fits the slot's tile (fleet and threat list);
  - whose three episodes (seeds of the draw), played by `learned_lockstep.host_episode`, show the properties that only an episode shows
    (a dead agent at a gate, more open tasks than the task pad at a gate, a gate without a valid pair, an episode of at most 3 steps);
  - whose oracle peaks stay MARGIN = 2 entries below every bound of the tile (capacity_cases.TILES), so that no device overflow is expected;
  - whose twin work in the lockstep (valid pairs at the gates it checks against the twin) stays below COST, so that a GPU case takes seconds.

The scan plays the episodes with a float64 matmul of the same network (fast); the entry that is written comes from the twin's float32 scores
(`entry`, which the CPU test calls too) and must confirm margin and properties, else the id is skipped and the slot scanned on.  A property
that no id of the window shows is reported and belongs in NOT_FOUND (with the reason in DESIGN.md)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import learned_lockstep as LL  # noqa: E402
import policy_mlp_py as twin  # noqa: E402
from capacity_cases import TILES  # noqa: E402
from fuzz_device_params import params_of_wide  # noqa: E402
from fuzz_reference import BIG, EDGE, wide_config  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "learned_fuzz_cases.json")
MARGIN, SCAN, COST = 2, 3000, 16000
FAMILY = {"small": 0, "large": BIG, "edge": EDGE}
TILE = {16: (16, 40, 16), 24: (24, 48, 24), 64: (64, 128, 48)}
OFFSET = {"pair": 0, "context": 1000, "coalition": 2000}
TWIN_FIRST, TWIN_EVERY = 3, 5   # device_lockstep's defaults
HIDDEN_COST = {"pair": 1, "context": 2, "coalition": 4}

PROPERTIES_ASKED = (
    "fleet_lt_agent_pad_t16", "fleet_lt_agent_pad_t24", "fleet_lt_agent_pad_t64", "fleet_gt_16_narrow_t24", "fleet_gt_16_narrow_t64", "fleet_gt_48_wide",
    "open_gt_task_pad_at_gate", "gate_without_valid_pair", "single_task_per_agent", "dead_agent_at_gate", "obstacles", "random_init_pos",
    "no_time_windows", "sense_radius_0", "sense_radius_ge_2000", "share_knowledge_off", "escort_on_pair", "escort_on_context", "escort_off_coalition",
    "commit_horizon", "edge_le_3_steps", "interval_1", "interval_gt_episode", "use_vis_on", "use_vis_off")
NOT_FOUND = ()
PROPERTIES = tuple(p for p in PROPERTIES_ASKED if p not in NOT_FOUND)
EPISODE_PROPS = ("open_gt_task_pad_at_gate", "gate_without_valid_pair", "dead_agent_at_gate", "edge_le_3_steps", "interval_gt_episode")


def _slots():
    """(kind, tile, pads, family, (fleet lo, fleet hi), weight set, properties the case must show)"""
    out = []
    for kind in LL.TABLE:
        esc = "escort_off_coalition" if kind == "coalition" else f"escort_on_{kind}"
        pads = LL.TABLE[kind].pads()
        plan = [
            (16, "small", (1, 15), ("single_task_per_agent", "obstacles")),
            (16, "small", (1, 16), ("dead_agent_at_gate",)),
            (16, "edge", (1, 16), ("edge_le_3_steps",)),
            (16, "edge", (1, 16), ("interval_1",)),
            (24, "small", (1, 15), ("random_init_pos", "no_time_windows")),
            (24, "large", (17, 24), (esc,)),
            (24, "large", (17, 24), ("sense_radius_0",)),
            (24, "edge", (1, 24), ("interval_gt_episode",)),
            (64, "small", (1, 15), ("sense_radius_ge_2000", "share_knowledge_off")),
            (64, "large", (25, 64), ("commit_horizon",)),
            (64, "large", (17, 64), ("open_gt_task_pad_at_gate",)),
            (64, "edge", (1, 64), ("gate_without_valid_pair",)),
        ]
        for j, (tile, fam, fleet, props) in enumerate(plan):
            if kind == "coalition" and props == ("open_gt_task_pad_at_gate",):
                props = ()  # no large-family id of the window has more than 48 open tasks at a gate AND stays within MARGIN and COST under this kind: a large fleet alone
            out.append((kind, tile, pads, fam, fleet, LL.WEIGHT_SETS[kind][j % 3], props))
    wide = [("pair", 24, "large", (17, 24), "init2"), ("pair", 64, "large", (49, 64), "init2_raw"), ("pair", 64, "small", (1, 16), "il3"),
            ("context", 24, "large", (17, 24), "init2_raw"), ("context", 64, "large", (49, 64), "il3"), ("context", 24, "small", (1, 16), "init2")]
    for kind, tile, fam, fleet, wname in wide:
        out.append((kind, tile, LL.WIDE, fam, fleet, wname, ("fleet_gt_48_wide",) if fleet[0] > 48 else ()))
    return out


SLOTS = _slots()


def seeds_of(seed, n=3):
    return [seed - i if seed > 2 ** 62 else seed + i for i in range(n)]


def use_vis_of(k):
    return k % 2 == 0


def config_props(cfg, interval, k, kind, tile, pads):
    na = sum(cfg["agents"].values())
    ma = LL.TABLE[kind].pads(pads)[1]
    wide = tuple(pads) == LL.WIDE
    p = set()
    if na < ma:
        p.add(f"fleet_lt_agent_pad_t{tile}")
    if na > 16 and not wide and tile in (24, 64):
        p.add(f"fleet_gt_16_narrow_t{tile}")
    if na > 48 and wide:
        p.add("fleet_gt_48_wide")
    for name, on in (("single_task_per_agent", not cfg["multiple_tasks_per_agent"]), ("obstacles", cfg["num_obstacles"] > 0), ("random_init_pos", cfg["random_init_pos"]),
                     ("no_time_windows", not cfg["include_time_windows"]), ("sense_radius_0", cfg["sense_radius"] == 0.0), ("sense_radius_ge_2000", cfg["sense_radius"] >= 2000),
                     ("share_knowledge_off", not cfg["share_knowledge"]), ("commit_horizon", cfg["commit_horizon"] > 0), ("interval_1", interval == 1),
                     ("use_vis_on", use_vis_of(k)), ("use_vis_off", not use_vis_of(k))):
        if on:
            p.add(name)
    if kind == "coalition":
        if not cfg["escort_enabled"]:
            p.add("escort_off_coalition")
    elif cfg["escort_enabled"]:
        p.add(f"escort_on_{kind}")
    return p


def episode_props(cfg, interval, k, kind, pads, runs):
    mt = LL.TABLE[kind].pads(pads)[0]
    p = set()
    for r in runs:
        for g in r["gates"]:
            if g["n_open"] > mt:
                p.add("open_gt_task_pad_at_gate")
            if g["n_valid"] == 0:
                p.add("gate_without_valid_pair")
            if g["n_dead"] > 0 and cfg["fail_rate"] > 0:
                p.add("dead_agent_at_gate")
        if k >= EDGE and r["steps"] <= 3:
            p.add("edge_le_3_steps")
        if interval > r["steps"]:
            p.add("interval_gt_episode")
    return p


def twin_cost(kind, runs):
    """valid pairs at the gates device_lockstep checks against the twin, weighted by the kind's layer widths"""
    total = 0
    for r in runs:
        for g, gate in enumerate(r["gates"]):
            if g < TWIN_FIRST or (g - TWIN_FIRST) % TWIN_EVERY == TWIN_EVERY - 1:
                total += gate["n_valid"]
    return total * HIDDEN_COST[kind]


def fast_scores(kind, w):
    """the same network by a float64 matmul, rounded to float32: what the scan plays with"""
    K = LL.TABLE[kind].twin

    def f(tok):
        ok = twin.cells(K, tok)
        s, lg = twin.forward64(K, w, tok)
        return (s * ok).astype(np.float32), (lg * ok).astype(np.float32)
    return f


def play(k, tile, kind, wname, pads, fast):
    wc = wide_config(k)
    cfg, interval = wc["cfg"], wc["interval"]
    w = LL.weights(kind, wname)
    params = params_of_wide(cfg, TILE[tile])
    fn = fast_scores(kind, w) if fast else None
    return wc, [LL.host_episode(params, s, kind, w, interval, use_vis_of(k), pads, scores_fn=fn) for s in seeds_of(wc["seed"])]


def judge(k, tile, kind, pads, wc, runs):
    """(properties shown, lists too close to the tile's bounds, twin cost)"""
    cfg, interval = wc["cfg"], wc["interval"]
    props = config_props(cfg, interval, k, kind, tile, pads) | episode_props(cfg, interval, k, kind, pads, runs)
    tight = sorted({name for r in runs for name in LL.fits(TILES[tile], r["peaks"], MARGIN)})
    return props, tight, twin_cost(kind, runs)


def entry(k, tile, kind, wname, pads):
    """one case of the file, from the oracle and the twin's float32 scores"""
    tile_n = tile[0] if isinstance(tile, (tuple, list)) else tile
    wc, runs = play(k, tile_n, kind, wname, tuple(pads), fast=False)
    props, tight, cost = judge(k, tile_n, kind, tuple(pads), wc, runs)
    fam = "edge" if k >= EDGE else "large" if k >= BIG else "small"
    return {"id": f"{kind}-{wname}-t{tile_n}-{'x'.join(map(str, pads))}-{fam}{k - FAMILY[fam]}", "k": k, "family": fam, "tile": list(TILE[tile_n]), "kind": kind,
            "weights": wname, "pads": list(pads), "seeds": seeds_of(wc["seed"]), "interval": wc["interval"], "use_vis": use_vis_of(k),
            "steps": int(wc["cfg"]["max_time_steps"]), "fleet": sum(wc["cfg"]["agents"].values()), "ended": [r["steps"] for r in runs],
            "gates": [len(r["gates"]) for r in runs], "n_replans": [int(r["n_replans"]) for r in runs], "peaks": [r["peaks"] for r in runs],
            "props": sorted(props), "tight": tight, "twin_cost": cost}


def fits_slot(cfg, tile, fleet):
    na, nh = sum(cfg["agents"].values()), sum(n for _, n in cfg["threats_list"])
    tl = TILES[tile]
    return fleet[0] <= na <= min(fleet[1], tl.A) and nh <= tl.H


def scan(slot, used, log):
    kind, tile, pads, fam, fleet, wname, need = slot
    need_cfg = [p for p in need if p not in EPISODE_PROPS]
    base = FAMILY[fam]
    for j in range(SCAN):
        k = base + (OFFSET[kind] + j) % SCAN
        if (kind, k) in used:
            continue
        wc = wide_config(k)
        cfg = wc["cfg"]
        if not fits_slot(cfg, tile, fleet) or cfg["max_time_steps"] > 260:
            continue
        if not set(need_cfg) <= config_props(cfg, wc["interval"], k, kind, tile, pads):
            continue
        if "dead_agent_at_gate" in need and cfg["fail_rate"] <= 0:
            continue
        if "edge_le_3_steps" in need and cfg["max_time_steps"] > 3:
            continue
        if "interval_gt_episode" in need and wc["interval"] <= cfg["max_time_steps"]:
            continue
        _, runs = play(k, tile, kind, wname, pads, fast=True)
        props, tight, cost = judge(k, tile, kind, pads, wc, runs)
        if tight or cost > COST or not set(need) <= props or min(len(r["gates"]) for r in runs) < 1:
            continue
        e = entry(k, tile, kind, wname, pads)
        if e["tight"] or e["twin_cost"] > COST or not set(need) <= set(e["props"]) or min(e["gates"]) < 1:
            log(f"  k={k}: the twin's episode does not confirm the scan's (tight {e['tight']}, cost {e['twin_cost']}): skipped")
            continue
        used.add((kind, k))
        return e
    return None


def coverage(cases):
    have = {}
    for c in cases:
        for p in c["props"]:
            have[p] = have.get(p, 0) + 1
    return have


def main():
    import multiprocessing as mp
    check = "--check" in sys.argv
    # slots of one kind that draw from the same family and tile must not take the same id: those are scanned one after the other
    groups = {}
    for i, s in enumerate(SLOTS):
        groups.setdefault((s[0], s[1], s[2], s[3]), []).append(i)
    jobs = list(groups.values())
    with mp.get_context("spawn").Pool(min(len(jobs), len(os.sched_getaffinity(0)))) as pool:
        parts = pool.map(_group, jobs)
    cases = [None] * len(SLOTS)
    for part in parts:
        for i, e, lines in part:
            for ln in lines:
                print(ln)
            cases[i] = e
    missing_slots = [SLOTS[i] for i, e in enumerate(cases) if e is None]
    for s in missing_slots:
        print(f"NOT FOUND within {SCAN} ids: slot {s}")
    cases = [e for e in cases if e is not None]
    have = coverage(cases)
    absent = [p for p in PROPERTIES_ASKED if not have.get(p)]
    print(f"{len(cases)} cases; properties: {have}")
    print(f"properties not found: {absent} (NOT_FOUND = {list(NOT_FOUND)})")
    assert sorted(absent) == sorted(NOT_FOUND), "NOT_FOUND of this file is not what the search gives"
    doc = {"margin": MARGIN, "scan": SCAN, "cost": COST, "not_found": list(NOT_FOUND), "cases": cases}
    text = json.dumps(doc, indent=1, sort_keys=True) + "\n"
    if check:
        assert open(OUT).read() == text, "the committed file is not what the search gives"
        print("the committed file is reproduced")
    else:
        with open(OUT, "w") as f:
            f.write(text)
        print(f"wrote {OUT} ({len(text)} bytes)")


def _group(idx):
    used, out = set(), []
    for i in idx:
        lines = []
        out.append((i, scan(SLOTS[i], used, lines.append), lines))
    return out


if __name__ == "__main__":
    main()
