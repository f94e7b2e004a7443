#!/usr/bin/env python3
"""Golden outcomes of the threshold probes, by RUNNING the reference (builder's container only; data only is written).

    python tools/gen_golden_thresholds.py [case ...]

Every probe group of tests/threshold_probes.py (the project's own code) is run on the reference env built as tools/gen_golden.py builds it
(make_env) and its records go to tests/golden/thr_<case>.npz as arrays `<group>_<field>`: the threshold id, its value, the side (-1 below,
0 at, +1 above), the sweep index, the positions written (float64), the reference's distance and squared sum, the outcome record.

Nothing is written unless every probe is shown to have reached its comparison:
  - every threshold has a probe on each side -1, 0, +1 (T1 per radius);
  - the recorded distance of a direct probe equals pred(thr), thr or succ(thr) bit for bit, according to its side;
  - the reference's outcomes on sides -1 and +1 differ, and the outcome on side 0 is the one the reference's operator dictates;
  - every T1 / T2 sweep holds a pair of probes whose squared sums are one ulp apart and whose outcomes differ;
  - the tied distances of T3 / T4 are equal as bit patterns, and the tied pair is returned in agent order.
"""
from __future__ import annotations

import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

from gen_golden import OUT, make_env  # noqa: E402  (installs refshim)

import threshold_probes as P  # noqa: E402

# threshold label -> (column of the outcome record that holds the comparison's result, its value where the comparison holds, the side-0 result
# the reference's operator dictates: True = the comparison holds at equality)
DECIDES = {
    "T1": (1, 1, True),               # dist <= sense_radius: known bit
    "T2": (1, 1, True),               # dist <= escort_radius: covered step
    "T3": (2, 3, True),               # dist <= r: all three fighters returned
    "T4:intercept": (0, 1, True),     # dist <= escort_intercept_radius: the threat turns to the fighter
    "T4:engaged": (0, 1, True),       # the same for the hunter that fights in the step: it fights the fighter (and not the recon)
    "T4:support": (0, 1, True),       # dist <= mutual_support_radius: a second defender, the engagement counts
    "T5": (1, 2, False),              # dist < max_speed: state 2
    "T6:engage": (3, 1, False),       # dist < engage_range: the fighter leaves state 1
    "T6:disengage": (3, 1, True),     # dist >= engage_range: the fighter leaves state 2
    "T7:leave": (1, 3, False),        # dist > max_speed + 5: state 3
    "T7:arrive": (1, 0, False),       # dist < max_speed + 5: state 0
}
# the comparison of these holds ABOVE the threshold, of the others below it
HOLDS_ABOVE = {"T6:disengage", "T7:leave"}


def refuse(why):
    raise SystemExit(f"gen_golden_thresholds: refusing to write: {why}")


def check(case, group, recs):
    """the conditions that keep a probe from being vacuous; returns the per-threshold side counts"""
    counts = {}
    by_thr = {}
    for r in recs:
        by_thr.setdefault((r["thr"], r["value"]), []).append(r)
    for (thr, value), rows in sorted(by_thr.items()):
        tag = f"{case} {group} {thr} at {value}"
        direct = [r for r in rows if r["k"] < 0]
        sweep = sorted((r for r in rows if r["k"] >= 0), key=lambda r: r["k"])
        if thr.endswith("tie"):
            for r in rows:
                if np.float64(r["outcome"][0]).tobytes() != np.float64(r["outcome"][1]).tobytes() or r["outcome"][0] != value or r["dist"] != value:
                    refuse(f"{tag}: the tied distances differ: {r['outcome']}")
                if r["outcome"][2] != 1:
                    refuse(f"{tag}: the reference did not put the first of the equidistant fighters first: {r['outcome']}")
            counts[(thr, value)] = {0: len(rows)}
            continue
        col, holds, at_equal = DECIDES[thr]
        sides = {s: [r for r in direct if r["side"] == s] for s in (-1, 0, 1)}
        for s, rs in sides.items():
            if not rs:
                refuse(f"{tag}: no probe on side {s}")
            for r in rs:
                if np.float64(r["dist"]).tobytes() != np.float64(P.at_side(value, s)).tobytes():
                    refuse(f"{tag} side {s}: the reference's distance is {r['dist']!r}, not {P.at_side(value, s)!r}")
        inside, outside = (1, -1) if thr in HOLDS_ABOVE else (-1, 1)
        for r in sides[inside]:
            if r["outcome"][col] != holds:
                refuse(f"{tag}: the comparison did not hold on side {inside}: {r['outcome']}")
        for r in sides[outside]:
            if r["outcome"][col] == holds:
                refuse(f"{tag}: the comparison held on side {outside}: {r['outcome']}")
        for r in sides[0]:
            if (r["outcome"][col] == holds) != at_equal:
                refuse(f"{tag}: at equality the reference gave {r['outcome']}, its operator says {'holds' if at_equal else 'does not hold'}")
        if thr == "T1":
            for r in rows:
                if r["outcome"][0] != 0 or r["outcome"][2] != 0:
                    refuse(f"{tag}: the task was known beforehand or the agent moved: {r['outcome']}")
        if thr == "T3":
            for r in rows:
                if np.float64(r["outcome"][0]).tobytes() != np.float64(r["outcome"][1]).tobytes():
                    refuse(f"{tag}: the tied distances differ")
                n = int(r["outcome"][2])         # the returned ids, then the id of the fighter on the radius: the tied pair in agent order, it last
                ids, on_radius = r["outcome"][3:3 + n].tolist(), r["outcome"][3 + n]
                if n < 2 or not ids[0] < ids[1] or (n == 3 and ids[2] != on_radius) or on_radius in ids[:2]:
                    refuse(f"{tag}: the returned ids {ids} do not keep the tied pair in agent order before the fighter on the radius")
        if thr in ("T1", "T2"):
            flips = 0
            for a, b in zip(sweep, sweep[1:]):
                if b["sqsum"] != a["sqsum"] + np.spacing(a["sqsum"]):
                    refuse(f"{tag}: sweep squared sums {a['sqsum']!r}, {b['sqsum']!r} are not one ulp apart")
                flips += a["outcome"][col] != b["outcome"][col]
            if flips != 1:
                refuse(f"{tag}: the sweep's outcome flips {flips} times")
        counts[(thr, value)] = {s: len(rs) for s, rs in sides.items()}
        if sweep:
            counts[(thr, value)]["sweep"] = len(sweep)
            counts[(thr, value)]["flip after k"] = next(a["k"] for a, b in zip(sweep, sweep[1:]) if a["outcome"][col] != b["outcome"][col])
    return counts


def main():
    only = sys.argv[1:]
    files = {}
    for case, groups in P.PLAN.items():         # every case is run and checked before the first file is written
        if only and case not in only:
            continue
        out = {}
        for group in groups:
            recs = P.run(P.GROUPS[group](make_env(case), seed=P.SEED))
            for key, n in check(case, group, recs).items():
                print(f"{case:18s} {group:8s} {key[0]:13s} thr {key[1]:6.1f}  probes per side {n}", flush=True)
            for k, v in P.pack(recs).items():
                out[f"{group}_{k}"] = v
        buf = io.BytesIO()
        np.savez_compressed(buf, **out)
        if buf.tell() > 100 * 1024:
            refuse(f"thr_{case}.npz would hold {buf.tell()} B, more than 100 KB")
        files[os.path.join(OUT, f"thr_{case}.npz")] = buf.getvalue()
    for path, data in files.items():
        with open(path, "wb") as f:
            f.write(data)
        print(path, len(data), "B", flush=True)


if __name__ == "__main__":
    main()
