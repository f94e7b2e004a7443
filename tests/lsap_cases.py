"""Cost matrices for the stand-alone LSAP probes of the environment tiles, and a counting restatement of scipy's solver.

Plain numpy, no GPU.  `cases(R, C)` is the deterministic case list of a tile with R agents and C task slots (the solver's limit is
R x C after scipy's transpose); `twin(cost)` is scipy's `rectangular_lsap` (1.15.3) with counters that say how deep a matrix drives
the search.  tests/test_lsap_cases_cpu.py pins the twin to the oracle (and to scipy where it is installed) and asserts that every tile's
set reaches the parts of the device solvers the simulation rarely does; tests/test_gpu_lsap_tiles.py feeds the sets to the device.
"""
import numpy as np

SEED = 20240607
TILES = {"tile16": (16, 40), "tile24": (24, 48), "tile64": (64, 128)}  # impl name of batched.lsap -> (R, C)
WAVE = 64  # register cost columns need one lane per column; the 64-agent tile evaluates costs on the fly beyond that


def shapes(R, C):
    """(nr, nc) of the set, nr > nc being transposed input: the tile's corners, one off them, the degenerate ones, one odd interior
    shape whose columns fit a wave (it runs the register solver on every tile, past the 16- and 48-row tuple boundaries), and on a tile
    wider than a wave 33 x 100 — with R x (R+1) and C x R the first, an interior and a transposed problem on the on-the-fly path."""
    r = (3 * R // 4) | 1
    out = [(R, R), (R, C), (C, R), (R - 1, R), (R, R + 1), (1, C), (R, 1), (1, 1), (r, ((r + min(C, WAVE)) // 2) | 1)]
    if C > WAVE:
        out.append((33, 100))
    assert len(set(out)) == len(out) and all(min(s) <= R and max(s) <= C for s in out)
    return out


def _feasible_inf(rng, k, nr, nc):
    """uniform costs, 60 % of them +inf, around a random finite perfect matching of the shorter side"""
    c = rng.random((k, nr, nc))
    hole = rng.random((k, nr, nc)) < 0.6
    for p in range(k):
        if nr <= nc:
            hole[p, np.arange(nr), rng.permutation(nc)[:nr]] = False
        else:
            hole[p, rng.permutation(nr)[:nc], np.arange(nc)] = False
    c[hole] = np.inf
    return c


def _family(name, rng, nr, nc):
    """cost[k, nr, nc] of one family at one shape"""
    near_square = abs(nr - nc) <= 1
    if name == "uniform":
        return rng.random((4, nr, nc))
    if name == "product":  # c[i][j] = (i+1)(j+1) and its reverse, each also with 1e-3 noise: every row's search scans every assigned row
        p = np.outer(np.arange(1, nr + 1), np.arange(1, nc + 1)).astype(np.float64)
        return np.stack([p, p[::-1, ::-1].copy(), p + 1e-3 * rng.random((nr, nc)), p[::-1, ::-1] + 1e-3 * rng.random((nr, nc))])
    if name == "rank1":
        return np.stack([np.outer(rng.uniform(1, 2, nr), rng.uniform(1, 2, nc)) for _ in range(3)])
    if name == "geom":  # the simulator's own cost shape: distance / max_coord - 0.6 urgency, 1e6 where the pair is not allowed
        k = 4
        a, t = rng.uniform(0, 1200, (k, nr, 1, 2)), rng.uniform(0, 1200, (k, 1, nc, 2))
        c = np.sqrt(((a - t) ** 2).sum(axis=3)) / 1200.0 - 0.6 * rng.random((k, 1, nc))
        c[rng.random((k, nr, nc)) < 0.25] = 1e6
        return c
    if name == "ties":
        k = 8 if near_square else 4
        c = rng.integers(0, 3, (k, nr, nc)).astype(np.float64)
        c[rng.random((k, nr, nc)) < 0.3] = 1e6
        return c
    if name == "negzero":
        c = rng.uniform(-1, 1, (4, nr, nc))
        c[rng.random((4, nr, nc)) < 0.2] = -0.0
        return c
    if name == "inf_sparse":
        return _feasible_inf(rng, 4, nr, nc)
    if name == "levels":
        # Every entry of a column (of scipy's matrix: the longer axis) costs the column's level, 0..3.  A level's columns go to one row
        # each in a single step; the row that finds them all taken scans every assigned row and ends in a tie between ALL free columns
        # of the next level, wherever they sit in `remaining` — in both 64-position chunks on a problem wider than a wave, which
        # `ties` does not reach: its rows take the lowest free column first, and those fill the far end of `remaining`.
        k = 4
        lev = rng.integers(0, 4, (k, 1, nc) if nr <= nc else (k, nr, 1)).astype(np.float64)
        return np.broadcast_to(lev, (k, nr, nc)).copy()
    raise KeyError(name)


FAMILIES = ("uniform", "product", "rank1", "geom", "ties", "negzero", "inf_sparse", "levels")
# Matrices on which a device solver once differed from the oracle stay here by name: (name, cost[k, nr, nc]) per tile limit (R, C).
NAMED = {}


def cases(R, C):
    """[(family, cost[k, nr, nc])]: every family at every shape of the tile, 3 to 8 problems each, the same on every call"""
    rng = np.random.default_rng(SEED + 1000 * R + C)
    out = [(f, np.ascontiguousarray(_family(f, rng, nr, nc))) for nr, nc in shapes(R, C) for f in FAMILIES]
    return out + list(NAMED.get((R, C), []))


def twin(cost):
    """scipy.optimize.linear_sum_assignment(cost) restated (rectangular_lsap.cpp; the scan over `remaining` as array operations: the
    sequential rule "lower, or equal and unassigned" picks the LAST unassigned position among the minima, else the FIRST minimum).
    Returns (row, col, counters):
      deepest          rows scanned by the longest search for one augmenting path (at most min(nr, nc))
      fast_rows        rows whose search ends in its first scan step
      assigned_ties    scan steps that continue the search with several (assigned) columns at the minimum
      deep_final_ties  last scan steps with several unassigned columns at the minimum, in a search of more than one row
      split_final_ties such last steps whose chosen column sits in a later 64-position chunk of `remaining` than another minimum
      split_fast_ties  one-step searches whose chosen column sits in a later 64-column chunk than another (assigned) minimum"""
    c = np.asarray(cost, dtype=np.float64)
    tr = c.shape[1] < c.shape[0]
    if tr:
        c = np.ascontiguousarray(c.T)
    nr, nc = c.shape
    u, v = np.zeros(nr), np.zeros(nc)
    path, col4row, row4col = np.full(nc, -1), np.full(nr, -1), np.full(nc, -1)
    stat = dict(deepest=0, fast_rows=0, assigned_ties=0, deep_final_ties=0, split_final_ties=0, split_fast_ties=0)
    for cur in range(nr):
        minval, i, sink, depth = 0.0, cur, -1, 0
        remaining = np.arange(nc - 1, -1, -1)
        SR, SC = np.zeros(nr, bool), np.zeros(nc, bool)
        spc = np.full(nc, np.inf)
        while sink == -1:
            SR[i] = True
            depth += 1
            r = minval + c[i, remaining] - u[i] - v[remaining]
            better = r < spc[remaining]
            path[remaining[better]] = i
            spc[remaining[better]] = r[better]
            s = spc[remaining]
            minval = s.min()
            if minval == np.inf:
                raise ValueError("cost matrix is infeasible")
            at_min = np.flatnonzero(s == minval)
            free = at_min[row4col[remaining[at_min]] == -1]
            index = free[-1] if len(free) else at_min[0]
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
                stat["deep_final_ties"] += depth > 1 and len(free) > 1
                # the solver that scans a wave's worth at a time (positions in a search, columns in a row's first step): the chosen
                # minimum lies in a later chunk than another column at the minimum
                stat["split_final_ties"] += int(depth > 1 and index // WAVE > at_min[0] // WAVE)
                stat["split_fast_ties"] += int(depth == 1 and j // WAVE > remaining[at_min].min() // WAVE)
            else:
                i = row4col[j]
                stat["assigned_ties"] += len(at_min) > 1
            SC[j] = True
            remaining[index] = remaining[-1]
            remaining = remaining[:-1]
        stat["deepest"] = max(stat["deepest"], depth)
        stat["fast_rows"] += depth == 1
        u[cur] += minval
        others = SR.copy()
        others[cur] = False
        u[others] += minval - spc[col4row[others]]
        v[SC] -= minval - spc[SC]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    if tr:
        order = np.argsort(col4row, kind="stable")
        return col4row[order].astype(np.int64), order.astype(np.int64), stat
    return np.arange(nr, dtype=np.int64), col4row.astype(np.int64), stat
