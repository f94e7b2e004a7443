"""The LSAP solvers of the environment tiles, stand-alone (batched.lsap(impl="tile16" | "tile24" | "tile64")): Sim<Tile16 / Tile24 /
Tile64>'s own instantiation of the register and on-the-fly solvers against the oracle's restatement of scipy, bit for bit, on the case
sets of tests/lsap_cases.py — which tests/test_lsap_cases_cpu.py shows to drive every search loop to its full depth — and on every
matrix the simulation itself solves in the oracle's episodes."""
import numpy as np
import pytest

import lsap_cases
import orc
from muavta_amd.params import params_for_case

pytestmark = pytest.mark.gpu

LIMITS = dict(lsap_cases.TILES, registers=(32, 64), lds=(64, 128))  # impl -> min(nr, nc) x max(nr, nc) it accepts


def impls_holding(nr, nc):
    return [impl for impl, (a, t) in LIMITS.items() if min(nr, nc) <= a and max(nr, nc) <= t]


def check_batch(batch, want_row, want_col, impls, tag):
    from muavta_amd.batched import lsap
    for impl in impls:
        row, col = lsap(batch, impl=impl)
        for k in range(len(batch)):
            assert np.array_equal(row[k], want_row[k]) and np.array_equal(col[k], want_col[k]), \
                f"{tag} problem {k} impl {impl}: rows {row[k].tolist()} cols {col[k].tolist()}, oracle {want_row[k].tolist()} {want_col[k].tolist()}"


@pytest.mark.parametrize("tile", sorted(lsap_cases.TILES))
def test_tile_solvers_equal_the_oracle(tile):
    for family, batch in lsap_cases.cases(*lsap_cases.TILES[tile]):
        nr, nc = batch.shape[1:]
        impls = impls_holding(nr, nc)
        assert tile in impls and "lds" in impls
        want = [orc.lsap(c) for c in batch]
        check_batch(batch, [w[0] for w in want], [w[1] for w in want], impls, f"{tile} {family} {nr}x{nc}")


def test_tile_solvers_on_the_simulators_own_matrices():
    for case, tile in (("WPS_hard_x2", "tile16"), ("WPS_escort24", "tile24"), ("WPS_burst64", "tile64")):
        by_shape = {}
        o = orc.OracleEnv(params_for_case(case))
        for seed in (0, 1):
            o.reset(seed)
            for _ in range(150):
                aa, ai = o.allocate(20, 1)
                shapes, costs, rows, cols = o.lsap_calls()
                off = ro = 0
                for nr, nc in shapes.tolist():
                    m = min(nr, nc)
                    by_shape.setdefault((nr, nc), []).append((costs[off:off + nr * nc].reshape(nr, nc), rows[ro:ro + m], cols[ro:ro + m]))
                    off += nr * nc; ro += m
                if o.step(aa, ai):
                    break
        assert by_shape, case
        for (nr, nc), calls in by_shape.items():
            assert tile in impls_holding(nr, nc), (case, nr, nc)
            check_batch(np.stack([c for c, _, _ in calls]), [r for _, r, _ in calls], [c for _, _, c in calls], (tile, "lds"), f"{case} {nr}x{nc}")


def test_tile_solvers_refuse_what_scipy_refuses():
    """scipy.optimize.linear_sum_assignment raises ValueError for an infeasible matrix and for NaN / -inf entries"""
    from muavta_amd.batched import lsap
    from muavta_amd.native import MuavtaError
    rng = np.random.default_rng(11)
    for tile, (R, C) in sorted(lsap_cases.TILES.items()):
        shapes = [(R, C), (C, R)] + ([(R, lsap_cases.WAVE)] if C > lsap_cases.WAVE else [])  # (the 64-agent tile: both of its solvers)
        for nr, nc in shapes:
            good = rng.random((3, nr, nc))
            want = [orc.lsap(c) for c in good]
            bad = good.copy()
            if nr <= nc:
                bad[1, nr // 2, :] = np.inf
            else:
                bad[1, :, nc // 2] = np.inf  # (a row of scipy's transposed matrix)
            with pytest.raises(MuavtaError, match="cost matrix 1 is infeasible"):
                lsap(bad, impl=tile)
            check_batch(good, [w[0] for w in want], [w[1] for w in want], (tile,), f"{tile} after an infeasible {nr}x{nc}")
            for entry in (np.nan, -np.inf):
                bad = good.copy()
                bad[2, nr - 1, nc - 1] = entry
                with pytest.raises(MuavtaError, match="invalid numeric"):
                    lsap(bad, impl=tile)
                check_batch(good, [w[0] for w in want], [w[1] for w in want], (tile,), f"{tile} after a refused {nr}x{nc}")
