"""The refusal paths of the C ABI (include/muavta.h), through raw calls so that the return code itself is asserted: every call below
is refused with MUAVTA_E_ARG or MUAVTA_E_STATE (and, where other tests match on the text, a message substring), none of them touches the
env state, and a handle that went through all of them afterwards computes what a fresh handle computes."""
import ctypes as C

import numpy as np
import pytest

from muavta_amd import native
from muavta_amd.batched import F, BatchedMultiUAVEnv, _vp
from muavta_amd.params import MuavtaRecord, params_for_case

pytestmark = pytest.mark.gpu

OK, E_ARG, E_STATE = 0, -1, -5
CASE, N = "WPS_hard", 4
MT, MA = 32, 16
OP_COUNT, OP_SET_QUEUE = 7, 6


def _changing_calls(env):
    """the calls of the test that do change the handle (both handles make them): reset, a whole-batch rollout, two sub-batch
    rollouts, a whole-batch rollout"""
    L, h = env.L, env.h
    seeds = np.arange(7, 7 + N, dtype=np.uint64)
    assert L.muavta_reset(h, _vp(seeds)) == OK
    yield "reset"
    assert L.muavta_rollout(h, None, 2, 20, 1, 1) == OK
    yield "rollout"
    assert L.muavta_set_parts(h, 2) == OK
    for p in range(2):
        assert L.muavta_rollout_part(h, p, 1, 20, 1, 1) == OK
    yield "rollout_part"
    assert L.muavta_rollout(h, None, 1, 20, 1, 1) == OK
    yield "rollout again"


def test_every_refusal_returns_its_code_and_leaves_the_handle_untouched():
    import torch

    env = BatchedMultiUAVEnv(params_for_case(CASE), N)
    L, h = env.L, env.h
    A, T, nA = env.A_tile, env.T, env.n_agents
    dev = torch.device("cuda", 0)
    tdt = {np.float32: torch.float32, np.uint8: torch.uint8, np.int32: torch.int32, np.uint64: torch.int64, np.float64: torch.float64}

    def tens(shapes):
        return {k: torch.zeros(sh, dtype=tdt[dt], device=dev) for k, (sh, dt) in shapes.items()}

    def refused(rc, code, text=None):
        assert rc == code, f"return code {rc}, expected {code}: {L.muavta_last_error(h).decode()}"
        if text is not None:
            assert text in L.muavta_last_error(h).decode()

    tok, ptok = tens(env.token_shapes("pair", MT, MA)), tens(env.token_shapes("pair", MT, MA))
    tok_ptrs = [C.c_void_p(tok[k].data_ptr()) for k in ("task_feats", "task_mask", "task_ids", "agent_feats", "agent_mask", "agent_ids", "edge_valid", "n_urgent")]
    ctx = torch.zeros((N, 8), dtype=torch.float32, device=dev)
    none_rows = np.full((N, A), -1, dtype=np.int32)
    zero_rows = np.zeros((N, A), dtype=np.int32)
    metrics = np.zeros((N, 64), dtype=np.float64)
    call_out, call_args = np.zeros(72, dtype=np.int32), np.zeros(8, dtype=np.int32)

    def spec(kind=0, mt=MT, ma=MA, gate=1, flags=1):
        return native.MuavtaScored(kind, mt, ma, gate, flags, 20, 1, 0)

    def rl_step(plan, part=0, **ptrs):
        rs = native.MuavtaRlStep()
        rs.plan, rs.part = plan, part
        for k, v in ptrs.items():
            setattr(rs, k, v.data_ptr())
        return L.muavta_rl_step_device(h, C.byref(rs))

    def rl_run(plan, part=0, max_steps=0, **ptrs):
        rr = native.MuavtaRlRun()
        rr.first.plan, rr.first.part, rr.max_steps = plan, part, max_steps
        for k, v in ptrs.items():
            setattr(rr if k.startswith("park_") else rr.first, k, v.data_ptr())
        return L.muavta_rl_run_device(h, C.byref(rr))

    def step_run(aa=None, ai=None, gate=1, max_steps=0):
        return L.muavta_step_run(h, _vp(aa), _vp(ai), gate, 20, max_steps, 1, None, None, None)

    part_calls = {
        "rollout_part": lambda p: L.muavta_rollout_part(h, p, 1, 20, 1, 1),
        "allocate_part": lambda p: L.muavta_allocate_part(h, p, 20, 1, None, None),
        "step_part": lambda p: L.muavta_step_part(h, p, None, None),
        "observe_part": lambda p: L.muavta_observe_part(h, p, *([None] * 7)),
        "rl_step part": lambda p: rl_step(spec(), part=p + 1),
        "rl_run part": lambda p: rl_run(spec(), part=p + 1),
    }

    # ---- before reset ----------------------------------------------------------------------------------------------------------------
    refused(L.muavta_step(h, _vp(none_rows), _vp(zero_rows)), E_STATE)
    refused(L.muavta_step_staged(h), E_STATE)
    refused(L.muavta_allocate(h, 20, 1, None, None), E_STATE)
    refused(L.muavta_rollout(h, None, 1, 20, 1, 1), E_STATE)
    refused(L.muavta_metrics(h, _vp(metrics)), E_STATE)
    refused(L.muavta_observe(h, None, None, None, None, None), E_STATE)
    refused(L.muavta_tokens_device(h, 0, MT, MA, *tok_ptrs, None, None), E_STATE)
    refused(L.muavta_context_device(h, 0, MT, C.c_void_p(ctx.data_ptr())), E_STATE)
    refused(L.muavta_call(h, 0, 0, _vp(call_args), -1.0, _vp(call_out)), E_STATE)
    refused(step_run(), E_STATE)
    refused(L.muavta_allocate_scored_device(h, C.byref(spec())), E_STATE)
    for name, call in part_calls.items():  # no parts set: refused as such, whatever else is wrong
        if "rl_" not in name:
            refused(call(0), E_ARG)
    assert L.muavta_set_parts(h, 2) == OK
    for name, call in part_calls.items():
        refused(call(0), E_STATE)
    assert L.muavta_set_parts(h, 0) == OK

    # ---- timing, around the calls that change the handle --------------------------------------------------------------------------------
    ms, hist = C.c_float(), np.zeros(64, dtype=np.float32)
    for stage in _changing_calls(env):
        if stage == "reset":
            refused(L.muavta_last_kernel_ms(h, C.byref(ms)), E_STATE)
            refused(L.muavta_kernel_ms_history(h, _vp(hist), 0), E_ARG)
            refused(L.muavta_kernel_ms_history(h, _vp(hist), 65), E_ARG)
            refused(L.muavta_kernel_ms_history(h, _vp(hist), 1), E_STATE)
            refused(L.muavta_launch_gaps_ms(h, _vp(hist), 1), E_ARG)
        elif stage == "rollout_part":  # part launches record no event pair
            refused(L.muavta_last_kernel_ms(h, C.byref(ms)), E_STATE)
            refused(L.muavta_kernel_ms_history(h, _vp(hist), 1), E_STATE)
        else:
            assert L.muavta_last_kernel_ms(h, C.byref(ms)) == OK and ms.value > 0
            refused(L.muavta_kernel_ms_history(h, _vp(hist), 3), E_STATE)  # (more than the launches so far)
    assert L.muavta_kernel_ms_history(h, _vp(hist), 2) == OK
    before = env.get_state().copy()

    # ---- action rows -------------------------------------------------------------------------------------------------------------------
    refused(L.muavta_step_lists(h, _vp(none_rows), _vp(zero_rows), 0), E_ARG)
    refused(L.muavta_step_lists(h, _vp(none_rows), _vp(zero_rows), 32768), E_ARG)
    bad_rows = none_rows.copy()
    bad_rows[2, 0] = nA
    refused(L.muavta_step_lists(h, _vp(bad_rows), _vp(zero_rows), A), E_ARG, "agent id")
    refused(L.muavta_step(h, _vp(bad_rows), _vp(zero_rows)), E_ARG, "agent id")
    refused(step_run(bad_rows, zero_rows), E_ARG, "agent id")
    first, count = env.part_range(1)
    part_bad = np.full((count, A), -1, dtype=np.int32)
    part_bad[count - 1, 1], part_bad[count - 1, 0] = nA + 3, 0
    refused(L.muavta_step_part(h, 1, _vp(part_bad), _vp(np.zeros((count, A), dtype=np.int32))), E_ARG, "agent id")
    refused(L.muavta_step_part(h, 1, _vp(part_bad), None), E_ARG)
    refused(step_run(none_rows, None), E_ARG)
    refused(step_run(None, zero_rows), E_ARG)
    refused(step_run(gate=4), E_ARG)
    refused(step_run(max_steps=-1), E_ARG)

    # ---- scored spec -------------------------------------------------------------------------------------------------------------------
    bad_specs = [spec(kind=3), spec(mt=0), spec(mt=129), spec(ma=65), spec(gate=4), spec(flags=8), spec(kind=2, flags=2)]
    for s in bad_specs:
        refused(L.muavta_allocate_scored_device(h, C.byref(s)), E_ARG)
        refused(rl_step(s), E_ARG)
        refused(rl_run(s), E_ARG)
    for missing in ("task_mask", "edge_valid"):
        some = {k: v for k, v in tok.items() if k != missing}
        refused(rl_step(spec(), **some), E_ARG)
        refused(rl_run(spec(), **some), E_ARG)
        refused(rl_run(spec(), **tok, **{"park_" + k: v for k, v in ptok.items() if k != missing}), E_ARG)
    refused(rl_run(spec(), max_steps=-1), E_ARG)

    # ---- release log on ----------------------------------------------------------------------------------------------------------------
    assert L.muavta_set_release_log(h, 1) == OK
    refused(rl_step(spec()), E_STATE)
    refused(rl_run(spec()), E_STATE)
    refused(step_run(), E_STATE)
    refused(L.muavta_step_part(h, 0, None, None), E_STATE)
    assert L.muavta_set_release_log(h, 0) == OK

    # ---- parts -------------------------------------------------------------------------------------------------------------------------
    for name, call in part_calls.items():
        refused(call(2), E_ARG)  # part = n_parts
    assert L.muavta_set_parts(h, 0) == OK
    for name, call in part_calls.items():
        refused(call(0), E_ARG)
    refused(L.muavta_set_parts(h, 9), E_ARG)
    refused(L.muavta_set_parts(h, N + 1), E_ARG)
    f_, c_ = C.c_int32(), C.c_int32()
    refused(L.muavta_part_range(h, 1, C.byref(f_), C.byref(c_)), E_ARG)
    assert L.muavta_set_parts(h, 2) == OK
    refused(L.muavta_part_range(h, 2, C.byref(f_), C.byref(c_)), E_ARG)
    refused(L.muavta_part_range(h, -1, C.byref(f_), C.byref(c_)), E_ARG)

    # ---- muavta_rollout_record -----------------------------------------------------------------------------------------------------------
    rings, obs = tens(env.record_shapes("pair", 1, MT, MA)), tens(env.obs_ring_shapes(1))

    def record(kind=-1, write_obs=1, token_rings=None, obs_rings=None):
        rec = MuavtaRecord()
        rec.kind, rec.max_tasks, rec.max_agents = kind, MT, MA
        for src in (token_rings or {}), (obs_rings or {}):
            for k, v in src.items():
                setattr(rec, k, v.data_ptr())
        return L.muavta_rollout_record(h, None, 1, 20, 1, write_obs, C.byref(rec))

    refused(record(), E_ARG)  # nothing to record
    refused(record(obs_rings={k: v for k, v in obs.items() if k != "obs_done"}), E_ARG)
    refused(record(obs_rings=obs, write_obs=0), E_ARG)
    refused(record(kind=3, token_rings=rings), E_ARG)
    refused(record(kind=0, token_rings={k: v for k, v in rings.items() if k != "s_wps"}), E_ARG)
    assert L.muavta_set_allocator(h, 5) == OK
    refused(record(kind=0, token_rings=rings), E_ARG, "Cap-Greedy / PI")
    assert L.muavta_set_allocator(h, 0) == OK
    w = {k: np.zeros(sh, dtype=np.float32) for k, sh in (("w0", (128, 25)), ("b0", 128), ("w1", (128, 128)), ("b1", 128), ("w2", (1, 128)), ("b2", 1))}
    mlp = native.MuavtaPairMlp(0, 128, 0.35, *[a.ctypes.data for a in w.values()])
    assert L.muavta_set_pair_policy(h, C.byref(mlp)) == OK
    assert L.muavta_set_allocator(h, 6) == OK
    refused(record(kind=0, token_rings=rings), E_ARG, "MLP-Pair")
    refused(L.muavta_set_pair_policy(h, None), E_STATE, "selected")
    assert L.muavta_set_allocator(h, 0) == OK
    assert L.muavta_set_pair_policy(h, None) == OK

    # ---- settings ------------------------------------------------------------------------------------------------------------------------
    refused(L.muavta_set_allocator(h, -1), E_ARG)
    refused(L.muavta_set_allocator(h, 7), E_ARG)
    refused(L.muavta_set_allocator(h, 6), E_STATE, "set_pair_policy")
    refused(L.muavta_pair_scores(h, None, None), E_STATE, "no policy")
    refused(L.muavta_set_pair_policy(h, C.byref(native.MuavtaPairMlp(0, 64, 0.35))), E_ARG, "hidden")
    refused(L.muavta_set_lanes(h, 3), E_ARG)
    refused(L.muavta_set_slot_cap(h, T + 1), E_ARG)
    refused(L.muavta_allreduce_metrics(h, _vp(metrics), 1, None, 0, _vp(metrics), None), E_STATE, "before muavta_comm_init")

    # ---- state access --------------------------------------------------------------------------------------------------------------------
    pos = np.zeros((N, nA, 2), dtype=np.float64)
    refused(L.muavta_get(h, F["AGENT_POS"], _vp(pos), pos.nbytes - 8), E_ARG, "need")
    refused(L.muavta_set(h, F["AGENT_POS"], _vp(pos), pos.nbytes + 8), E_ARG, "need")
    ids = np.zeros((N, T), dtype=np.int32)
    refused(L.muavta_set(h, F["TASK_ID"], _vp(ids), ids.nbytes), E_ARG, "read-only")
    refused(L.muavta_get(h, F["RELEASE_LOG"], _vp(pos), pos.nbytes), E_STATE)
    state, rng = env.get_state(), env.get_rng()
    refused(L.muavta_get_state(h, _vp(state), state.nbytes - 1), E_ARG)
    refused(L.muavta_set_state(h, _vp(state), state.nbytes + 1), E_ARG)
    refused(L.muavta_get_rng(h, _vp(rng), rng.nbytes - 4), E_ARG)
    refused(L.muavta_set_rng(h, _vp(rng), rng.nbytes + 4), E_ARG)

    # ---- muavta_call ---------------------------------------------------------------------------------------------------------------------
    refused(L.muavta_call(h, 0, OP_COUNT, _vp(call_args), -1.0, _vp(call_out)), E_ARG)
    refused(L.muavta_call(h, N, 0, _vp(call_args), -1.0, _vp(call_out)), E_ARG)
    refused(L.muavta_call(h, 0, 0, _vp(np.array([nA] + [0] * 7, dtype=np.int32)), -1.0, _vp(call_out)), E_ARG)
    refused(L.muavta_call(h, 0, OP_SET_QUEUE, _vp(np.array([0, 7] + [0] * 6, dtype=np.int32)), -1.0, _vp(call_out)), E_ARG)

    # ---- muavta_lsap_impl (no handle: the message is the thread's) -------------------------------------------------------------------------
    cost = np.zeros(65 * 129, dtype=np.float64)
    row, col = np.zeros(128, dtype=np.int64), np.zeros(128, dtype=np.int64)
    assert L.muavta_lsap_impl(0, _vp(cost), 0, 2, 2, _vp(row), _vp(col), 0) == E_ARG
    assert L.muavta_lsap_impl(0, _vp(cost), 1, 65, 129, _vp(row), _vp(col), 0) == E_ARG
    assert L.muavta_lsap_impl(0, _vp(cost), 1, 33, 64, _vp(row), _vp(col), 2) == E_ARG
    for nr, nc, impl, limit in ((17, 40, 3, "16 x 40"), (16, 41, 3, "16 x 40"), (25, 48, 4, "24 x 48")):  # an env tile's solver, one past its limit
        assert L.muavta_lsap_impl(0, _vp(cost), 1, nr, nc, _vp(row), _vp(col), impl) == E_ARG
        assert limit in L.muavta_last_error(None).decode()
    assert L.muavta_lsap_impl(0, _vp(cost), 1, 2, 2, _vp(row), _vp(col), 6) == E_ARG
    assert "unknown solver" in L.muavta_last_error(None).decode()
    cost[3] = np.nan
    assert L.muavta_lsap_impl(0, _vp(cost), 1, 2, 2, _vp(row), _vp(col), 0) == E_ARG
    assert "invalid numeric" in L.muavta_last_error(None).decode()

    # ---- none of it touched the handle ---------------------------------------------------------------------------------------------------
    torch.cuda.synchronize()
    assert np.array_equal(env.get_state(), before)
    assert not env.get("ERROR").any()
    fresh = BatchedMultiUAVEnv(params_for_case(CASE), N)
    for _ in _changing_calls(fresh):
        pass
    rows = {}
    for e in (env, fresh):
        aa, ai = e.allocate(20, True)
        rows[e] = (aa.copy(), ai)
    assert np.array_equal(rows[env][0], rows[fresh][0]) and np.array_equal(rows[env][1], rows[fresh][1])
    junk = rows[env][0]
    terminated = 0
    for n in range(N):  # an id behind the -1 terminator is never looked at
        ends = np.nonzero(junk[n] < 0)[0]
        if len(ends) and ends[0] + 1 < A:
            junk[n, ends[0] + 1] = nA + 40
            terminated += 1
    assert terminated, "no row of the plan ends in front of the last column"
    assert L.muavta_step(h, _vp(junk), _vp(rows[env][1])) == OK
    fresh.step(*rows[fresh])
    assert np.array_equal(env.get_state(), fresh.get_state())
    assert np.array_equal(env.get_rng(), fresh.get_rng())
    assert not env.get("ERROR").any()
