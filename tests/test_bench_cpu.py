"""bench.py's bookkeeping that needs no GPU: the roofline block of the JSON line (labels as VERDICT r4 item 6 asked) is well formed for the three
tiles, `frac` is exactly algorithmic bytes per launch / the kernel's launch duration / HBM peak, and the PMC-derived fields (measured HBM traffic, VALU-port
occupancy, lane utilisation) appear only when profiles/pmc_traffic.json was collected on exactly the kernel sources of this tree (source hash) — a figure
taken on other sources must never be attached to a new build's line."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

TILES = (("WPS_hard_x2", 4096, 16, 32, 16), ("WPS_escort24", 4096, 24, 48, 24), ("WPS_burst64", 1024, 64, 128, 64))


@pytest.mark.parametrize("case,envs,tile,max_tasks,n_agents", TILES)
def test_roofline_block_is_well_formed_and_follows_8d(case, envs, tile, max_tasks, n_agents):
    kernel_ms, iso_ms, per_step = 4.5, 2.5, 2.4
    r = bench.roofline(case, envs, tile, kernel_ms, iso_ms, per_step, 2, max_tasks, n_agents)
    json.dumps(r)  # (goes into the one JSON line)
    B = bench.ALGO_BYTES_PER_ENV_STEP[tile]
    assert r["bound"] == "issue" and r["unit"] == "GB/s" and r["peak"] == bench.HBM_PEAK_GBS == 8000.0 and r["kernel"] == "k_rollout"
    assert r["achieved"] == pytest.approx(envs * bench.HORIZON * B / (kernel_ms * 1e-3) / 1e9, rel=1e-12) and r["frac"] == pytest.approx(r["achieved"] / 8000.0, rel=1e-12)
    assert r["isolated"]["frac"] == pytest.approx(envs * bench.HORIZON * B / (iso_ms * 1e-3) / 1e9 / 8000.0, rel=1e-12)
    assert r["device_frac"] == pytest.approx(envs * bench.HORIZON * B / (per_step * 1e-3) / 1e9 / 8000.0, rel=1e-12) and r["launches_in_flight"] == 2
    floor = max_tasks * 84 + max_tasks + n_agents * (36 + 4 * ((max_tasks + 31) // 32)) + 30 + 4 * n_agents
    assert r["hbm_floor_bytes_per_env_step"] == floor < B
    e = bench.pmc_entry(case, envs)
    if e is None:  # the PMC passes were taken on other kernel sources: nothing measured may be attached
        assert r["traffic"] is None and r["issue_frac"] is None and r["lane_util"] is None and r["hbm_measured_frac"] is None and r["issue"] is None
    else:
        assert e["source_hash"] == bench.source_hash() == r["issue"]["source_hash"]
        assert r["traffic"] == e["bytes_per_launch"] > 0 and 0.0 < r["issue_frac"] <= 1.0 and 0.0 < r["lane_util"] <= 1.0
        assert r["hbm_measured_frac"] == pytest.approx(e["bytes_per_launch"] / (kernel_ms * 1e-3) / 1e9 / 8000.0, rel=1e-12)
        assert os.path.isfile(os.path.join(ROOT, "profiles", e["profile"]))  # the summary the figure comes from is committed


def test_pmc_figures_of_other_kernel_sources_are_not_attached(monkeypatch):
    monkeypatch.setattr(bench, "source_hash", lambda: "0" * 16)
    for case, envs, tile, mt, na in TILES:
        assert bench.pmc_entry(case, envs) is None and bench.measured_traffic(case, envs) is None
        r = bench.roofline(case, envs, tile, 3.0, None, None, 1, mt, na)
        assert r["traffic"] is None and r["issue"] is None and r["frac"] is not None and "isolated" not in r and "device_frac" not in r


class _ObsStandIn:
    """observe() of a BatchedMultiUAVEnv of the headline tile (dtypes and shapes as muavta_amd.batched returns them), filled from `seed`"""

    def __init__(self, n, seed=0):
        self.n, self.rng = n, np.random.default_rng(seed)

    def observe(self):
        n, r = self.n, self.rng
        return {"tasks": r.random((n, 40, 21), dtype=np.float32), "legal_mask": r.random((n, 16, 40)) < 0.5, "mask": r.random((n, 40)) < 0.5,
                "agents": r.random((n, 16, 9), dtype=np.float32), "event_flags": r.random((n, 5), dtype=np.float32)}


@pytest.mark.parametrize("n", [4096, 32768])
def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path, n):
    """--dump-outputs: float32 / float64 .npy files only, the whole batch while it fits the budget, else the same seeded sample of rows in
    every array and on every run (two dumps of the same batch are identical)."""
    metrics = np.random.default_rng(1).random((n, 30))
    seeds = np.arange(n, dtype=np.uint64)
    dumps = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), _ObsStandIn(n), metrics, seeds, True)
        dumps.append({f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = dumps
    assert set(a) == {"metrics", "seeds", "obs_tasks", "obs_legal_mask", "obs_mask", "obs_agents", "obs_event_flags"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in a) <= 64e6
    rows = a["seeds"].astype(np.int64)
    assert len({len(v) for v in a.values()}) == 1 and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["metrics"], metrics[rows])
    assert (len(rows) == n) == (n == 4096)
    bench.dump_outputs(str(tmp_path / "m"), None, metrics, seeds, False)  # (no observation write: metrics and seeds only)
    assert sorted(os.listdir(tmp_path / "m")) == ["metrics.npy", "seeds.npy"]
