"""The learned allocator modes ('mlp_pair', 'mlp_context_pair', 'mlp_coalition', the (64, 48) token pads, the RL transition rings) against the
ORACLE on random configurations: the cases of tests/golden/learned_fuzz_cases.json (tools/find_learned_fuzz_cases.py), each one
configuration of tests/fuzz_reference.py::wide_config with 3 envs, through tests/learned_lockstep.py.  No tolerance except the two score
bounds of the kinds' own modules (4 spacings of score_clamp; test_gpu_mlp_coalition.SCORE_BOUND), which the lockstep imports.

An env is left out only when the device flagged it (ERROR) AND the oracle's own lists at that step exceed the tile's bound; at most one case
in eight per kind may lose an env that way (the selection keeps every list 2 entries below the bounds: none is expected)."""
import json
import os

import numpy as np
import pytest

import learned_lockstep as LL
import orc
from capacity_cases import TILES
from fuzz_device_params import params_of_wide
from fuzz_reference import wide_config
from test_gpu_parity import Snapshot, compare

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "learned_fuzz_cases.json")) as _f:
    CASES = json.load(_f)["cases"]
IDS = [c["id"] for c in CASES]
INDEX = {c["id"]: n for n, c in enumerate(CASES)}
RING_CASES = [c for c in CASES if c["kind"] in ("pair", "context") and tuple(c["pads"]) == LL.NARROW]  # the other combinations are refused by design
EXTRA_PATHS = {c["id"] for kind in ("pair", "context") for c in [c for c in RING_CASES if c["kind"] == kind][:2]}  # parts and lanes: the first two per kind
_REF = {}
LOST = {kind: set() for kind in LL.TABLE}     # cases that lost an env to a real overflow
TOTALS = {kind: dict(envs=0, twin_gates=0, skipped=0, steps=0) for kind in LL.TABLE}


def _setup(c):
    cfg = wide_config(c["k"])["cfg"]
    tile = tuple(c["tile"])
    return params_of_wide(cfg, tile), tile, LL.weights(c["kind"], c["weights"]), np.array(c["seeds"], dtype=np.uint64), tuple(c["pads"])


def _handle(c, n=3):
    p, tile, w, seeds, pads = _setup(c)
    return LL.make_env(p, n, c["kind"], w, pads, tile), p, w, seeds, pads


def reference(c):
    """the lockstep of a case, run once and shared by the three tests"""
    if c["id"] not in _REF:
        env, p, w, seeds, pads = _handle(c)
        try:
            oracles = [orc.OracleEnv(p) for _ in seeds]
            _REF[c["id"]] = LL.device_lockstep(env, oracles, seeds, c["kind"], w, c["interval"], c["use_vis"], pads, tag=c["id"])
        except AssertionError as exc:
            _REF[c["id"]] = exc
        finally:
            env.close()
        r = _REF[c["id"]]
        if not isinstance(r, AssertionError):
            t = TOTALS[c["kind"]]
            t["envs"] += len(seeds) - len(r["flagged"]); t["twin_gates"] += r["n_twin_gates"]; t["skipped"] += len(r["flagged"]); t["steps"] += r["n_steps"]
    r = _REF[c["id"]]
    if isinstance(r, AssertionError):
        raise AssertionError(f"lockstep: {r}")
    return r


def comparable(c, res):
    """the envs of the case that take part: all, unless the device flagged one whose oracle lists outgrow the tile at that step"""
    tl = TILES[c["tile"][0]]
    for i, (step, code, now) in res["flagged"].items():
        over = LL.fits(tl, now, 0)
        assert over, f"{c['id']} seed {c['seeds'][i]}: the device flagged ERROR {code} at step {step}, the oracle's lists {now} fit the tile {tl}"
        print(f"{c['id']} seed {c['seeds'][i]}: left out, ERROR {code} at step {step}: the oracle's {over} outgrow the tile ({now})")
        LOST[c["kind"]].add(c["id"])
    n_kind = sum(1 for x in CASES if x["kind"] == c["kind"])
    assert len(LOST[c["kind"]]) * 8 <= n_kind, f"{c['kind']}: {sorted(LOST[c['kind']])} of {n_kind} cases lost an env to an overflow"
    return [i for i in range(len(c["seeds"])) if i not in res["flagged"]]


def check_final(env, c, res, rows, metrics, tag, check_obs):
    """metrics, n_replans and every field of `env` against what each oracle held when its episode ended (= the lockstep's rows at that step)"""
    snap = Snapshot(env)
    for i in rows:
        f = res["final"][i]
        o = f["oracle"]
        assert np.array_equal(metrics[i], o.metrics()) and np.array_equal(metrics[i], f["metrics"]), f"{tag} seed {c['seeds'][i]}: metrics columns {np.nonzero(metrics[i] != o.metrics())[0].tolist()}"
        assert int(snap.SCALARS[i, 23]) == o.dims()["n_replans"] == f["n_replans"], f"{tag} seed {c['seeds'][i]}: n_replans"
        assert np.array_equal(snap.SCALARS[i], f["scalars"]), f"{tag} seed {c['seeds'][i]}: SCALARS row against the lockstep's"
        compare(snap, i, o, f"{tag} seed {c['seeds'][i]} final state", check_obs=check_obs)
        if LL.TABLE[c["kind"]].escort:
            assert np.array_equal(snap.AGENT_MISC[i, :o.A, 4], o.agent_commit_until()), f"{tag} seed {c['seeds'][i]}: commit locks"


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_lockstep_vs_oracle(c):
    res = reference(c)
    rows = comparable(c, res)
    for i in rows:
        f = res["final"][i]
        assert f is not None and f["steps"] == c["ended"][i] and len(res["gates"][i]) == c["gates"][i], \
            f"{c['id']} seed {c['seeds'][i]}: {f['steps']} steps, {len(res['gates'][i])} gates; the file has {c['ended'][i]}, {c['gates'][i]}"
        assert np.array_equal(f["metrics"], f["oracle"].metrics()), f"{c['id']} seed {c['seeds'][i]}: metrics at the end of the episode"
        assert int(f["scalars"][23]) == f["oracle"].dims()["n_replans"] == c["n_replans"][i], f"{c['id']} seed {c['seeds'][i]}: n_replans"
    t = TOTALS[c["kind"]]
    print(f"{c['id']}: {len(rows)} envs, {res['n_steps']} env steps, {res['n_twin_gates']} gates against the twin; {c['kind']} so far: {t}")


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_fused_rollout_vs_oracle(c):
    res = reference(c)
    rows = comparable(c, res)
    write_obs = INDEX[c["id"]] % 2 == 0
    env, p, w, seeds, pads = _handle(c)
    try:
        env.rollout(seeds, c["steps"], c["interval"], c["use_vis"], write_obs)
        check_final(env, c, res, rows, env.rollout_metrics(), f"{c['id']} fused (write_obs {write_obs})", write_obs)
        if c["id"] not in EXTRA_PATHS:
            return
        env.reset(seeds)                      # sub-batches
        env.set_parts(2)
        for part in range(2):
            env.rollout_part(part, c["steps"], c["interval"], c["use_vis"], True)
        env.wait_part(-1)
        env.sync()
        check_final(env, c, res, rows, LL.device_metrics(env), f"{c['id']} two parts", True)
        env.set_parts(0)
    finally:
        env.close()
    two, _, _, _, _ = _handle(c)              # two lanes: the same batch twice, back to back
    try:
        two.set_lanes(2)
        for _ in range(2):
            two.rollout(seeds, c["steps"], c["interval"], c["use_vis"], True)
        back, last = two.rollout_metrics(back=1), two.rollout_metrics()
        for i in rows:
            assert np.array_equal(back[i], res["final"][i]["metrics"]), f"{c['id']} seed {c['seeds'][i]}: the first lane's metrics"
        check_final(two, c, res, rows, last, f"{c['id']} two lanes", True)
    finally:
        two.close()


def _record(env, c, seeds):
    """il.rl_record (which plans with the visibility map); a case that plans without it goes through the call il.rl_record wraps, with
    the two tensors it adds derived the same way"""
    import torch
    from muavta_amd import il
    if c["use_vis"]:
        out = il.rl_record(env, seeds, n_steps=c["steps"], interval=c["interval"], noise_std=0)
    else:
        G = min(c["steps"], 64)
        dev = torch.device("cuda", env.device_index)
        tdt = {np.float32: torch.float32, np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64}
        out = {name: torch.empty(shape, dtype=tdt[dtype], device=dev) for name, (shape, dtype) in env.rl_record_shapes(G).items()}
        env.rollout_rl_record(seeds, c["steps"], c["interval"], False, out)
        env.sync()
        out["valid"] = torch.arange(G, device=dev)[:, None] < out["n_gates"].clamp(max=G)[None, :]
        diff = out["s_wps_after"] - out["s_wps_before"]
        out["step_reward"] = torch.div(diff, torch.full_like(diff, 20.0))
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("c", RING_CASES, ids=[c["id"] for c in RING_CASES])
def test_rl_rings_vs_oracle(c):
    """slot g of the rings = the env's g-th gate of the lockstep: its step, the stand-alone logits (tied to the twin there), the oracle's
    selected mask, done flags and (S_WPS after the planned step - S_WPS before the plan) / 20 (OracleEnv.rl_run, test_gpu_rl_record.py)"""
    res = reference(c)
    rows = comparable(c, res)
    env, p, w, seeds, pads = _handle(c)
    try:
        R = _record(env, c, seeds)
        check_final(env, c, res, rows, env.rollout_metrics(), f"{c['id']} recorded", False)
    finally:
        env.close()
    G = R["step"].shape[0]
    for i in rows:
        gates = res["gates"][i]
        tag = f"{c['id']} seed {c['seeds'][i]}"
        assert int(R["n_gates"][i]) == len(gates), f"{tag}: {int(R['n_gates'][i])} gates recorded, the lockstep saw {len(gates)}"
        assert np.array_equal(R["valid"][:, i], np.arange(G) < len(gates)), f"{tag}: valid"
        assert np.all(R["step"][len(gates):, i] == -1), f"{tag}: slots behind the last gate"
        for g, gate in enumerate(gates[:G]):
            assert int(R["step"][g, i]) == gate["step"], f"{tag} slot {g}: gate at step {int(R['step'][g, i])}, the oracle's at {gate['step']}"
            assert np.array_equal(R["logits"][g, i].view(np.uint32), gate["logits"].view(np.uint32)), f"{tag} slot {g}: logits"
            assert np.array_equal(R["selected"][g, i], gate["selected"]), f"{tag} slot {g}: selected mask"
            assert int(R["done"][g, i]) == gate["done"], f"{tag} slot {g}: done {int(R['done'][g, i])} vs {gate['done']}"
            assert R["s_wps_before"][g, i] == gate["s_before"] and R["s_wps_after"][g, i] == gate["s_after"], f"{tag} slot {g}: S_WPS"
            assert R["step_reward"][g, i] == (gate["s_after"] - gate["s_before"]) / 20.0, f"{tag} slot {g}: step reward"
