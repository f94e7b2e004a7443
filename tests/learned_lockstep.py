"""The host reference of an episode in a learned allocator mode (a helper, not a test): which oracle call is the planner of 'mlp_pair',
'mlp_context_pair' and 'mlp_coalition' (`TABLE`), the oracle alone along such an episode (`host_episode`) and a device handle in the mode
beside one oracle per env, compared at every step (`device_lockstep`).

The reference of a learned step is composed from parts that are pinned elsewhere: the oracle's token builders, context vector, scored
allocator and step (the `scored` leg of tests/fuzz_device.py, tests/test_oracle_golden.py) and the host twin of the forward pass
(tests/policy_mlp_py.py, exact up to the logits).  `TABLE` restates per kind which of them the mode chains — the chain the
test_fused_equals_stepwise_equals_scored_chain tests drive on the device — and tests/test_learned_lockstep_cpu.py pins it against the
reference's recorded episodes without a device.

The only device value that enters the reference in `device_lockstep` is the float32 score of a logit: the logit is compared with the twin
bit for bit and the score is held to the kind's bound against the float64 evaluation of that logit before the oracle plans with it, so the
two sides cannot part on a near-tie and nothing else is compared with a tolerance."""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import orc  # noqa: E402
import policy_mlp_py as twin  # noqa: E402

TOKEN_KINDS = {"pair": 0, "pair_raw": 1, "escort": 2}
NARROW, WIDE = (32, 16), (64, 48)
TOKEN_KEYS = ("task_feats", "task_mask", "task_ids", "agent_feats", "agent_mask", "agent_ids", "edge_valid", "n_urgent")
PEAKS = ("queue", "events", "pending", "escorts", "slots", "open")
BOUND_OF = {"queue": "Q", "events": "E", "pending": "R", "escorts": "A", "slots": "T", "open": "T"}  # fields of capacity_cases.Tile
WEIGHT_SETS = {"pair": ("init2", "init2_raw", "il3"), "context": ("init2", "init2_raw", "il3"), "coalition": ("init2", "ac3", "wide")}


def _scored_row(gate, kw):
    """(gate number, oracle flags) of the row of fuzz_device.SCORED with this gate and these keywords: the numbers are taken from there"""
    from fuzz_device import GATE, SCORED
    rows = [r for r in SCORED if r[0] == gate and r[1] == kw]
    assert rows, (gate, kw)
    return GATE[gate], rows[0][4]


@dataclass(frozen=True)
class Planner:
    name: str         # the kind
    mode: str         # set_allocator(...)
    twin: twin.Kind   # the forward pass
    escort: bool      # escort tokens (48, 16) whatever the pads; else 'pair' / 'pair_raw' by the weight set, at the handle's pads
    gate: str         # the callers' replan gate
    kw: tuple         # the keywords of BatchedMultiUAVEnv.allocate_scored of the same plan, as items

    @property
    def gate_flags(self):
        return _scored_row(self.gate, dict(self.kw))

    def token_kind(self, w):
        return "escort" if self.escort else ("pair_raw" if w["raw_features"] else "pair")

    def pads(self, pads=None):
        return (48, 16) if self.escort else tuple(pads or NARROW)


TABLE = {
    "pair": Planner("pair", "mlp_pair", twin.PAIR, False, "trainer", (("edge_valid_only", True),)),
    "context": Planner("context", "mlp_context_pair", twin.CONTEXT, False, "trainer", (("edge_valid_only", True),)),
    "coalition": Planner("coalition", "mlp_coalition", twin.COALITION, True, "escort", (("edge_valid_only", False), ("commit", True))),
}


def weights(kind, name):
    return twin.load_weights(TABLE[kind].twin, name)


def oracle_tokens(o, kind, w, pads=None):
    """the policy's input of the oracle's current state: the token dict, plus 'context' for the context kind"""
    P = TABLE[kind]
    mt, ma = P.pads(pads)
    k = TOKEN_KINDS[P.token_kind(w)]
    tok = o.tokens(k, mt, ma)
    if P.twin.context:
        tok["context"] = o.context(k, mt)
    return tok


def oracle_plan(o, kind, w, interval, use_vis, scores, pads=None):
    """the kind's planner on the oracle with these float32 scores -> (act_agent, act_index, selected, replanned)"""
    P = TABLE[kind]
    mt, ma = P.pads(pads)
    gate, flags = P.gate_flags
    t = o.dims()["time_steps"]
    aa, ai, sel = o.allocate_scored(interval, int(bool(use_vis)), gate, TOKEN_KINDS[P.token_kind(w)], mt, ma, flags, scores=scores)
    return aa, ai, sel, o.scalars_last_plan() == t


def twin_scores(kind, w):
    """scores_fn of host_episode: the twin's float32 scores (numpy's tanh / exp) and logits of one env's tokens"""
    return lambda tok: twin.forward(TABLE[kind].twin, w, {k: v for k, v in tok.items() if k in twin.TRACE_NAMES})


def counters(o):
    from capacity_cases import counters as c
    return c(o)


def fits(tl, peaks, margin=0):
    """the lists of `peaks` that do not stay `margin` entries below the bounds of capacity_cases.Tile `tl` (empty: the tile holds the episode)"""
    return [name for name in PEAKS if peaks[name] > getattr(tl, BOUND_OF[name]) - margin]


class Peaks:
    """the longest the lists a device tile bounds get along an episode (capacity_cases.counters / within: the slot need of a step is the ids
    held before it plus the ids it creates)"""

    def __init__(self, o):
        self.c = counters(o)
        self.v = dict(queue=self.c["queue"], events=max(self.c["events"], self.c["drained"]), pending=self.c["pending"], escorts=self.c["escorts"],
                      slots=self.c["held"], open=self.c["open"])

    def stepped(self, o):
        n, c, v = counters(o), self.c, self.v
        now = dict(queue=n["queue"], events=max(n["events"], n["drained"]), pending=n["pending"], escorts=n["escorts"],
                   slots=max(c["held"] + n["ids"] - c["ids"], n["held"]), open=n["open"])
        for k in v:
            v[k] = max(v[k], now[k])
        self.c = n
        return now


def host_episode(params, seed, kind, w, interval, use_vis, pads=None, scores_fn=None, lazy=True):
    """The oracle alone through an episode of the kind: per step tokens -> scores_fn(tokens) -> (scores, logits) -> the kind's planner ->
    step.  `lazy`: scores_fn is only consulted at the steps whose gate (OracleEnv.gate) fires — a plan that the gate refuses reads no score
    — and the planner's own gate bit must agree with it.  -> dict: gates (step, logits, selected, and what the policy saw of the state:
    live agent rows, open task columns, open tasks in all, valid pairs, dead agents), metrics, n_replans, steps, peaks."""
    P = TABLE[kind]
    scores_fn = scores_fn or twin_scores(kind, w)
    mt, ma = P.pads(pads)
    gate = P.gate_flags[0]
    o = orc.OracleEnv(params)
    o.reset(int(seed))
    peaks = Peaks(o)
    gates, t = [], 0
    while not (o.dims()["terminated"] or o.dims()["truncated"]) and t < params.max_time_steps:
        fire = o.gate(gate, interval) if lazy else True
        if fire:
            tok = oracle_tokens(o, kind, w, pads)
            scores, logits = scores_fn(tok)
        else:
            scores = np.zeros((ma, mt), np.float32)
        n_open = o.dims()["n_open"]
        aa, ai, sel, replanned = oracle_plan(o, kind, w, interval, use_vis, scores, pads)
        assert not lazy or replanned == fire, f"t={t}: OracleEnv.gate says {fire}, the planner's gate {replanned}"
        if replanned:
            ev = twin.cells(P.twin, tok)
            gates.append(dict(step=t, logits=logits, selected=sel, n_agents=int((tok["agent_mask"] == 0).sum()), n_tasks=int((tok["task_mask"] == 0).sum()),
                              n_open=n_open, n_valid=int(ev.sum()), n_dead=int((o.agents()[0][:, 2] == -1).sum())))
        o.step(aa, ai)
        peaks.stepped(o)
        t += 1
    return dict(gates=gates, metrics=o.metrics(), n_replans=o.dims()["n_replans"], steps=t, peaks=dict(peaks.v))


def score64(kind, w, logits):
    """the float64 evaluation of the SAME float32 logits: tanh(logit) * score_clamp, or sigmoid(clip(logit))"""
    return TABLE[kind].twin.score64(w, np.asarray(logits, np.float64))


def score_bound(kind, w):
    """the bound of the kind's GPU module on |score - score64(logit)|, imported from there"""
    if kind == "coalition":
        from test_gpu_mlp_coalition import SCORE_BOUND
        return SCORE_BOUND
    return 4 * float(np.spacing(np.float32(w["score_clamp"])))  # test_gpu_mlp_pair.test_tanhf_over_its_range: 4 spacings of score_clamp


def make_env(params, n, kind, w, pads=None, tile=None):
    """a device handle in the kind's mode (a tile with fewer than 40 slots is fuzz_device's capped 16-agent tile)"""
    from fuzz_device import make_env as mk
    env = mk(params, n, tile) if tile is not None else mk(params, n, (0, 40, 0))
    if not TABLE[kind].escort and pads is not None and tuple(pads) != NARROW:
        env.set_token_pads(*pads)
    env.set_pair_policy(twin.as_state_dict(w))
    env.set_allocator(TABLE[kind].mode)
    return env


def device_metrics(env):
    """muavta_metrics of every env; a capacity flag somewhere in the batch (the rows are filled all the same) is the caller's to handle"""
    from test_gpu_mlp_pair import metrics_of
    return metrics_of(env)


def device_lockstep(env, oracles, seeds, kind, w, interval, use_vis, pads=None, tag="", twin_first=3, twin_every=5):
    """`env`, a handle in the kind's mode, beside one oracle per env, from reset to the end of every env's episode.  At every step of every env
    whose episode has not ended: tokens (+ context) equal the oracle's; the stand-alone pair_scores gives the logits — equal to the twin's on the
    oracle's tokens at the env's first `twin_first` gates and every `twin_every`-th after —, unevaluated cells 0 and every score within the
    kind's bound of the float64 evaluation of its own logit; env.allocate in the mode stages what the oracle's planner returns for the device's
    scores (muavta_allocate returns no gate bit and no selected mask: the gate is compared through n_replans after the call, through every
    field after the step and, for the pair kinds, through the rings of the recording rollout); after step_staged every field and the
    observation (test_gpu_parity.compare), for the coalition kind the commit locks too.

    An env the device flags (ERROR) stops being compared: `flagged[i]` = (step, code, the oracle's peaks there).  An env whose episode has
    ended is no longer compared while the device keeps stepping it; its metrics row, SCALARS row and full state are taken at the step it ended.
    -> dict(gates=[per env: list of dict(step, logits, selected)], final=[per env: dict(metrics, scalars, n_replans, steps, oracle)],
            flagged={}, n_twin_gates, n_steps)"""
    from test_gpu_parity import Snapshot, compare
    P = TABLE[kind]
    n = len(oracles)
    mt, ma = P.pads(pads)
    kname = P.token_kind(w)
    bound = score_bound(kind, w)
    env.reset(np.asarray(seeds, dtype=np.uint64))
    for i, o in enumerate(oracles):
        o.reset(int(seeds[i]))
    peaks = [Peaks(o) for o in oracles]
    gates = [[] for _ in range(n)]
    final, flagged = [None] * n, {}
    live = [True] * n
    n_twin = n_steps = 0
    snap = Snapshot(env)
    for i, o in enumerate(oracles):
        if snap.ERROR[i]:
            flagged[i], live[i] = (0, int(snap.ERROR[i]), dict(peaks[i].v)), False
        else:
            compare(snap, i, o, f"{tag} seed {seeds[i]} after reset")
    t = 0
    while any(live):
        # 1. the policy's inputs
        got = env.tokens(kname, mt, ma)
        ctx = env.context(kname, mt) if P.twin.context else None
        want = {}
        for i, o in enumerate(oracles):
            if not live[i]:
                continue
            want[i] = oracle_tokens(o, kind, w, pads)
            for key in TOKEN_KEYS:
                gv = int(got[key][i]) if key == "n_urgent" else got[key][i]
                assert np.array_equal(np.asarray(gv), np.asarray(want[i][key])), f"{tag} seed {seeds[i]} t={t}: tokens: {key}"
            if ctx is not None:
                assert np.array_equal(ctx[i], want[i]["context"]), f"{tag} seed {seeds[i]} t={t}: context vector {ctx[i]} vs {want[i]['context']}"
        # 2. the stand-alone forward pass (leaves the state untouched)
        scores, logits = env.pair_scores(want_logits=True)
        assert scores.shape == (n, ma, mt)
        for i in want:
            ev = twin.cells(P.twin, want[i])
            assert not scores[i][~ev].any() and not logits[i][~ev].any(), f"{tag} seed {seeds[i]} t={t}: unevaluated cells"
            worst = float(np.abs(scores[i].astype(np.float64) - score64(kind, w, logits[i]))[ev].max(initial=0.0))
            assert worst <= bound, f"{tag} seed {seeds[i]} t={t}: |score - score64(logit)| = {worst:.3e} (bound {bound:.3e})"
        # 3. the plan in the mode beside the oracle's planner on the device's scores
        aa, ai = env.allocate(interval, use_vis)
        reps = env.get("SCALARS")[:, 23]
        plans = {}
        for i, o in enumerate(oracles):
            if not live[i]:
                continue
            s_before = o.metrics()[4]
            oa, oi, sel, replanned = oracle_plan(o, kind, w, interval, use_vis, scores[i], pads)
            kk = len(oa)
            assert np.array_equal(aa[i][:kk], oa) and np.all(aa[i][kk:] == -1) and np.array_equal(ai[i][:kk], oi), \
                f"{tag} seed {seeds[i]} t={t}: plan {aa[i][:kk + 2]} / {ai[i][:kk + 2]} vs {oa} / {oi}"
            assert int(reps[i]) == o.dims()["n_replans"], f"{tag} seed {seeds[i]} t={t}: n_replans after the plan {int(reps[i])} vs {o.dims()['n_replans']}"
            if replanned:
                g = len(gates[i])
                if g < twin_first or (g - twin_first) % twin_every == twin_every - 1:
                    _, tl = twin.forward(P.twin, w, {k: v for k, v in want[i].items() if k in twin.TRACE_NAMES})
                    diff = logits[i].view(np.uint32) != tl.view(np.uint32)
                    assert not diff.any(), f"{tag} seed {seeds[i]} t={t} gate {g}: {int(diff.sum())} logits differ from the host twin"
                    n_twin += 1
                gates[i].append(dict(step=t, logits=logits[i].copy(), selected=sel, s_before=s_before))
            plans[i] = (oa, oi, replanned)
        # 4. the step
        env.step_staged()
        snap = Snapshot(env)
        m = None
        for i, o in enumerate(oracles):
            if not live[i]:
                continue
            oa, oi, replanned = plans[i]
            done = o.step(oa, oi)
            now = peaks[i].stepped(o)
            n_steps += 1
            d = o.dims()
            if replanned:
                gates[i][-1].update(s_after=o.metrics()[4], done=int(bool(d["terminated"])) | (int(bool(d["truncated"])) << 1))
            if snap.ERROR[i]:
                flagged[i], live[i] = (t + 1, int(snap.ERROR[i]), now), False
                continue
            compare(snap, i, o, f"{tag} seed {seeds[i]} t={t + 1}")
            if P.escort:
                assert np.array_equal(snap.AGENT_MISC[i, :o.A, 4], o.agent_commit_until()), f"{tag} seed {seeds[i]} t={t + 1}: commit locks"
            if done or d["terminated"] or d["truncated"]:
                m = device_metrics(env) if m is None else m
                final[i] = dict(metrics=m[i].copy(), scalars=snap.SCALARS[i].copy(), n_replans=d["n_replans"], steps=t + 1, oracle=o,
                                state={name: getattr(snap, name)[i].copy() for name in Snapshot.NAMES})
                live[i] = False
        t += 1
        assert t <= env.params.max_time_steps, f"{tag}: an episode runs past max_time_steps"
    return dict(gates=gates, final=final, flagged=flagged, n_twin_gates=n_twin, n_steps=n_steps)
