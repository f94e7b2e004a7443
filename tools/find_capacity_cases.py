#!/usr/bin/env python3
"""Seed search for tests/capacity_cases.py, on the CPU oracle alone; writes tests/golden/capacity_cases.json.

  python tools/find_capacity_cases.py [--natural N] [--other-modes M] [--procs P]

For every constructed scenario (builder x tile x fits / overflow) the first seed whose oracle trace passes capacity_cases.check_trace; for the natural
episodes the first seeds among N whose deepest queue is exactly Q / more than Q under the Hungarian allocator (and the deepest queue of M seeds under each of
the other three allocators), and the WPS_escort24 / WPS_escort seeds whose pending-reveal list peaks at, below and past R of their tile; benign neighbours (episodes the tile holds); for the slot-cap test three seeds per tile with the oracle's bounds on the smallest
cap, the first of them an episode whose bounds meet and that stays at its peak slot need for several steps."""
import argparse
import json
import multiprocessing as mp
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import capacity_cases as cc  # noqa: E402

CONSTRUCTED = [("queue_call", ("fits", "overflow")), ("queue_list", ("fits", "overflow")), ("queue_steps", ("fits", "overflow")),
               ("events", ("fits", "overflow")), ("pending", ("fits", "overflow")), ("queue_then_events", ("overflow",)), ("escorts_full", ("fits",))]
NATURAL_CASES = {16: ["WPS_hard_x2", "full"], 24: ["WPS_escort24", "full"], 64: ["WPS_burst64", "full"]}
SLOT_CASE = {16: "WPS_hard_x2", 24: "WPS_escort24", 64: "WPS_burst64"}


def first_seed(builder, tile, kind, tries=400):
    for seed in range(1, tries):
        sc = cc.Scenario(builder, tile, kind, seed)
        try:
            trace, _ = cc.run_on_oracle(sc)
        except (ValueError, IndexError):
            continue
        ok, why = cc.check_trace(sc, trace)
        if ok:
            return seed, why
    return None, "no seed"


def _peaks(args):
    import orc
    case, tile, seeds = args
    o = orc.OracleEnv(cc.params(case, tile))
    out = []
    for s in seeds:
        sc = cc.Scenario("benign", tile, "benign", s, case)
        trace, _ = cc.run_on_oracle(sc, o)
        fine = all(i == 0 or cc.within(sc.tl, b, a, True) for i, (_, b, a) in enumerate(trace))
        held = [a["held"] for _, _, a in trace]
        out.append((s, max(a["queue"] for _, _, a in trace), max(a["pending"] for _, _, a in trace), fine, held.count(max(held))))
    return out


def natural_rows(n, procs):
    import orc
    orc.lib()
    rows = {}
    with mp.get_context("spawn").Pool(procs) as pool:
        for tile, cases in NATURAL_CASES.items():
            for case in cases:
                chunk = max(1, n // (procs * 4))
                jobs = [(case, tile, list(range(i, min(i + chunk, n)))) for i in range(0, n, chunk)]
                rows[(tile, case)] = [r for part in pool.map(_peaks, jobs) for r in part]
    return rows


def _mode_peaks(args):
    import orc
    case, tile, mode, seeds = args
    o = orc.OracleEnv(cc.params(case, tile))
    return [(s, cc.natural_peaks(case, tile, s, mode, o)) for s in seeds]


NEXT_TILE = {16: 24, 24: 64}
PENDING_ROUTES = [(24, "WPS_escort24", "hungarian_gated"), (24, "WPS_escort24", "urgency_pair"), (16, "WPS_escort", "urgency_pair")]
OTHER_MODES = ("urgency_pair", "urgency_coalition", "hungarian_gated")


def pending_rows(n, procs):
    """The registry's natural routes to R.  WPS_escort24 on its own 24-agent tile: under the gated Hungarian its list peaks at exactly 88 in a third of the
    seeds, under Urgency-Pair a few seeds pass it.  WPS_escort on the 16-agent tile under Urgency-Pair: nearly every seed passes 48.  An overflow seed is one
    whose episode the NEXT tile holds (that is where rollout(escalate=True) re-runs it) and whose queues stay within this one (so the first code is 4)."""
    out = []
    with mp.get_context("spawn").Pool(procs) as pool:
        for tile, case, mode in PENDING_ROUTES:
            jobs = [(case, tile, mode, list(range(i, min(i + 100, n)))) for i in range(0, n, 100)]
            r = [x for part in pool.map(_mode_peaks, jobs) for x in part]
            R, Q, R2 = cc.TILES[tile].R, cc.TILES[tile].Q, cc.TILES[NEXT_TILE[tile]].R
            out.append({"tile": tile, "next_tile": NEXT_TILE[tile], "case": case, "mode": mode, "searched": n,
                        "fits": [s for s, pk in r if pk["pending"] == R and pk["queue"] <= Q][:4],
                        "overflow": [s for s, pk in r if R < pk["pending"] <= R2 and pk["queue"] <= Q and pk["events"] <= cc.TILES[tile].E and pk["slots"] <= cc.TILES[tile].T][:4],
                        "below": [s for s, pk in r if pk["pending"] < R and pk["queue"] <= Q][:4]})
            print(f"pending_natural tile {tile} {case} {mode}: {out[-1]}", flush=True)
    return out


def queue_rows_other_modes(n, procs):
    """deepest natural queue per (tile, case) under the allocators other than the Hungarian one (which natural_rows covers with every counter)"""
    out = []
    with mp.get_context("spawn").Pool(procs) as pool:
        for tile, cases in NATURAL_CASES.items():
            for case in cases:
                for mode in OTHER_MODES:
                    jobs = [(case, tile, mode, list(range(i, min(i + 50, n)))) for i in range(0, n, 50)]
                    r = [x for part in pool.map(_mode_peaks, jobs) for x in part]
                    out.append({"tile": tile, "case": case, "mode": mode, "searched": n, "deepest_queue": max(pk["queue"] for _, pk in r)})
                    print(f"natural queue tile {tile} {case} {mode}: deepest {out[-1]['deepest_queue']} in {n} seeds", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--natural", type=int, default=6000)
    ap.add_argument("--other-modes", type=int, default=1000, help="seeds per case for the natural-queue search under the other allocators")
    ap.add_argument("--procs", type=int, default=max(1, min(8, len(os.sched_getaffinity(0)))))
    a = ap.parse_args()
    doc = {"tiles": {str(k): v._asdict() for k, v in cc.TILES.items()}, "scenarios": [], "natural_searched": a.natural, "slot_seeds": {}}
    for tile in cc.TILES:
        for builder, kinds in CONSTRUCTED:
            for kind in kinds:
                seed, why = first_seed(builder, tile, kind)
                print(f"{builder:18s} {kind:9s} tile {tile}: seed {seed} ({why})", flush=True)
                if seed is not None:
                    doc["scenarios"].append({"builder": builder, "tile": tile, "kind": kind, "seed": seed, "note": why})
    rows = natural_rows(a.natural, a.procs)
    for tile, tl in cc.TILES.items():
        found = {}
        for case in NATURAL_CASES[tile]:
            for s, q, pend, fine, _ in rows[(tile, case)]:
                if q == tl.Q and fine:
                    found.setdefault(("queue_natural", "fits"), (case, s, f"peak queue {q}"))
                if q > tl.Q:
                    found.setdefault(("queue_natural", "overflow"), (case, s, f"peak queue {q}"))
        for (builder, kind), (case, s, why) in sorted(found.items()):
            print(f"{builder:18s} {kind:9s} tile {tile}: {case} seed {s} ({why})", flush=True)
            doc["scenarios"].append({"builder": builder, "tile": tile, "kind": kind, "seed": s, "case": case, "note": why})
        for kind in ("fits", "overflow"):
            if ("queue_natural", kind) not in found:
                doc.setdefault("natural_not_found", []).append({"builder": "queue_natural", "tile": tile, "kind": kind, "cases": NATURAL_CASES[tile], "searched": a.natural})
                print(f"queue_natural      {kind:9s} tile {tile}: none among {a.natural} seeds of {NATURAL_CASES[tile]}", flush=True)
        # benign neighbours: the first seeds of each case that stay within the tile
        for case in (cc.QUEUE_CASE, "full", "slow"):
            if (tile, case) in rows:
                src = rows[(tile, case)]
            else:
                src = _peaks((case, tile, list(range(64))))
            doc.setdefault("benign", {}).setdefault(str(tile), {})[case] = [s for s, q, pend, fine, _ in src if fine][:8]
        case = SLOT_CASE[tile]
        # first the episodes whose two bounds meet (the smallest cap is known then, and is the slot count the episode stays at), longest stay first
        src = [(r, cc.slot_bounds(case, tile, r[0], cc.INTERVAL[case])) for r in rows[(tile, case)][:256] if r[3]]
        src = sorted(src, key=lambda rb: (rb[1][0] != rb[1][1], -rb[0][4], rb[0][0]))
        src = src[:1] + ([x for x in src[1:] if x[1][0] != x[1][1]] + src[1:])[:2]  # ... and two whose bounds differ, where there are any
        doc["slot_seeds"][str(tile)] = {"case": case, "seeds": [r[0] for r, _ in src], "steps_at_peak": [r[4] for r, _ in src], "bounds": [list(b) for _, b in src]}
        print(f"slot seeds tile {tile}: {doc['slot_seeds'][str(tile)]}", flush=True)
    doc["natural_pending"] = pending_rows(min(a.natural, 3000), a.procs)
    doc["natural_queue_other_modes"] = queue_rows_other_modes(a.other_modes, a.procs)
    with open(cc.GOLDEN, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
