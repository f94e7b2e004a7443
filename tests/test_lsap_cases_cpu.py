"""The LSAP case sets of tests/lsap_cases.py, without a GPU: the counting twin gives the oracle's (and scipy's) assignments on every
case, and every tile's set drives the search as deep as the conditions below say.  The conditions are properties of the inputs and of
the reference alone; tests/test_gpu_lsap_tiles.py relies on them when it feeds the same sets to the device solvers."""
import functools

import numpy as np
import pytest

import lsap_cases
import orc

TILE_NAMES = sorted(lsap_cases.TILES)


@functools.lru_cache(maxsize=None)
def solved(tile):
    """[(family, cost[nr, nc], row, col, counters)] of every problem of the tile's set, by the twin (computed once per tile)"""
    out = []
    for family, batch in lsap_cases.cases(*lsap_cases.TILES[tile]):
        assert batch.ndim == 3 and batch.dtype == np.float64 and 3 <= len(batch) <= 8, (tile, family, batch.shape)
        for c in batch:
            out.append((family, c) + lsap_cases.twin(c))
    return out


@pytest.mark.parametrize("tile", TILE_NAMES)
def test_twin_equals_the_oracle(tile):
    for family, c, row, col, _ in solved(tile):
        orow, ocol = orc.lsap(c)
        assert np.array_equal(row, orow) and np.array_equal(col, ocol), (tile, family, c.shape)


@pytest.mark.parametrize("tile", TILE_NAMES)
def test_twin_equals_scipy(tile):
    opt = pytest.importorskip("scipy.optimize")
    for family, c, row, col, _ in solved(tile):  # transposed shapes (nr > nc) included
        srow, scol = opt.linear_sum_assignment(c)
        assert np.array_equal(row, srow) and np.array_equal(col, scol), (tile, family, c.shape)


@pytest.mark.parametrize("tile", TILE_NAMES)
def test_case_sets_drive_the_search_to_full_depth(tile):
    R, C = lsap_cases.TILES[tile]
    probs = solved(tile)
    assert len(probs) == sum(len(b) for _, b in lsap_cases.cases(R, C))  # no case skipped or filtered
    first, again = lsap_cases.cases(R, C), lsap_cases.cases(R, C)  # the same list on every call
    assert len(first) == len(again) and all(f == g and np.array_equal(a, b) for (f, a), (g, b) in zip(first, again))
    by_shape = {}
    for family, c, _, _, stat in probs:
        assert min(c.shape) <= R and max(c.shape) <= C
        assert stat["deepest"] <= min(c.shape)
        by_shape.setdefault(c.shape, []).append(stat["deepest"])
    assert set(by_shape) == set(lsap_cases.shapes(R, C))
    for shape, deepest in by_shape.items():  # at every shape some search scans every row
        assert max(deepest) == min(shape), (tile, shape, max(deepest))
    assert sum(s["assigned_ties"] for *_, s in probs) >= 10
    assert sum(s["deep_final_ties"] for *_, s in probs) >= 5
    assert any(s["fast_rows"] for *_, s in probs) and any(s["fast_rows"] < min(c.shape) for _, c, _, _, s in probs)
    shapes = [c.shape for _, c, *_ in probs]
    assert any(nr > nc for nr, nc in shapes)  # transposed input
    assert any(nc == C for _, nc in shapes) and any(nr == R for nr, _ in shapes)
    if C > lsap_cases.WAVE:  # the 64-column mask boundary, the first problem beyond it, and a transposed problem beyond it
        assert {(64, 64), (63, 64), (64, 65), (33, 100), (128, 64)} <= set(shapes)
        # ties that span the 64-wide chunks the on-the-fly solver scans in: at the end of a deep search (`levels` alone gets there: a
        # build of that solver which ignored such a tie gave the oracle's answers on every other family) and in a row's single first step
        assert sum(s["split_final_ties"] for *_, s in probs) >= 5
        assert sum(s["split_fast_ties"] for *_, s in probs) >= 5
