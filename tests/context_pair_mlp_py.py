"""Host twin of the device's MLP-ContextPair forward pass (csrc/sim/policy.inc) — the arithmetic contract of DESIGN.md §7.1, restated
with numpy over `pair_mlp_py.fma32`.

ContextPairHybrid(use_attention=False): pair_mlp = Linear(58|41, 192) - ReLU - Linear(192, 192) - ReLU - Linear(192, 1) over
cat([agent row, task row, a_pool, t_pool, context]).  Exact up to the logits:

  pools     for each feature column d: s = 0.0f; s = s + x[row][d] in float32 over the rows whose mask is 0 (non-pad), ascending row;
            pool[d] = s / float32(max(count, 1)), one correctly rounded float32 division.  a_pool: the 16 agent rows, t_pool: the 32
            task rows.
  context   an input: what muavta_context(kind, 32) returns (pinned bit-exact against build_context_summary elsewhere).
  layer 1   ONE float32 fma chain per output from the bias over a_pool, t_pool, context, the agent row, the task row — in this order,
            ascending within each.  The state_dict's columns come in the reference's cat order (agent, task, a_pool, t_pool, context):
            `device_columns` is the permutation the packing step applies.
  then      ReLU, layer 2, layer 3 and the score as in pair_mlp_py.
"""
from __future__ import annotations

import numpy as np

import pair_mlp_py as base
from pair_mlp_py import f32, f64, linear, relu  # noqa: F401

HIDDEN = 192


def dims(raw):
    """(agent features, task features, context floats)"""
    return (11, 9, 1) if raw else (12, 13, 8)


def device_columns(raw):
    """device input k -> state_dict column: a_pool, t_pool, context first (env-uniform), then the agent row, then the task row"""
    da, dt, c = dims(raw)
    pair, pre = da + dt, da + dt + c
    return np.array([k + pair if k < pre else k - pre for k in range(pair + pre)], dtype=np.int64)


def pool(x, mask):
    """masked mean of the rows of x [R, D] (mask 0 = a real row): float32 adds in ascending row order from 0.0f, one float32 division"""
    x, mask = np.asarray(x, f32), np.asarray(mask)
    s = np.zeros(x.shape[1], f32)
    count = 0
    for r in range(x.shape[0]):
        if not mask[r]:
            s = (s + x[r]).astype(f32)
            count += 1
    return (s / f32(max(count, 1))).astype(f32)


def prefix(agent_feats, agent_mask, task_feats, task_mask, context):
    """the env-uniform head of layer 1's input row: a_pool, t_pool, context"""
    return np.concatenate([pool(agent_feats, agent_mask), pool(task_feats, task_mask), np.asarray(context, f32).reshape(-1)]).astype(f32)


def pair_logits(w, x):
    """x [P, K] float32 in DEVICE order (a_pool, t_pool, context, agent row, task row) -> logits [P] float32"""
    raw = w["w0"].shape[1] == 41
    w0 = np.ascontiguousarray(w["w0"][:, device_columns(raw)])
    h = relu(linear(w0, w["b0"], x))
    h = relu(linear(w["w1"], w["b1"], h))
    return linear(w["w2"], w["b2"], h)[:, 0]


def rows(pre, af, tf, ii, jj):
    return np.concatenate([np.broadcast_to(pre[None, :], (len(ii), len(pre))), af[ii], tf[jj]], axis=1).astype(f32)


def forward(w, agent_feats, agent_mask, task_feats, task_mask, context, edge_valid):
    """Token tensors of ONE env -> (scores, logits) [MA, MT] float32; 0 where edge_valid is 0 (those pairs are not evaluated)."""
    af, tf, ev = np.asarray(agent_feats, f32), np.asarray(task_feats, f32), np.asarray(edge_valid)
    ii, jj = np.nonzero(ev != 0)
    logits = np.zeros(ev.shape, f32)
    scores = np.zeros(ev.shape, f32)
    if len(ii):
        lg = pair_logits(w, rows(prefix(af, agent_mask, tf, task_mask, context), af, tf, ii, jj))
        logits[ii, jj] = lg
        scores[ii, jj] = (np.tanh(lg) * f32(w["score_clamp"])).astype(f32)
    return scores, logits


def forward_batch(w, tok, context):
    """the twin over every env of a token dict: (scores, logits) [N, 16, 32]; one chain evaluation for all valid pairs of the batch"""
    ev = tok["edge_valid"] != 0
    logits = np.zeros(ev.shape, f32)
    scores = np.zeros(ev.shape, f32)
    xs, at = [], []
    for n in range(ev.shape[0]):
        ii, jj = np.nonzero(ev[n])
        if len(ii):
            pre = prefix(tok["agent_feats"][n], tok["agent_mask"][n], tok["task_feats"][n], tok["task_mask"][n], context[n])
            xs.append(rows(pre, tok["agent_feats"][n], tok["task_feats"][n], ii, jj))
            at.append((np.full(len(ii), n), ii, jj))
    if xs:
        lg = pair_logits(w, np.concatenate(xs))
        nn, ii, jj = (np.concatenate(c) for c in zip(*at))
        logits[nn, ii, jj] = lg
        scores[nn, ii, jj] = (np.tanh(lg) * f32(w["score_clamp"])).astype(f32)
    return scores, logits


def forward64(w, agent_feats, agent_mask, task_feats, task_mask, context, edge_valid):
    """The same net in float64, pooling included, on the float32 tokens and the float32 context, in the reference's column order:
    the yardstick `scores64` of the fixtures.  -> (scores, logits) [MA, MT] float64"""
    af, tf, ev = np.asarray(agent_feats, f64), np.asarray(task_feats, f64), np.asarray(edge_valid)
    am, tm = (np.asarray(agent_mask) == 0).astype(f64)[:, None], (np.asarray(task_mask) == 0).astype(f64)[:, None]
    a_pool = (af * am).sum(0) / max(am.sum(), 1.0)
    t_pool = (tf * tm).sum(0) / max(tm.sum(), 1.0)
    MA, MT = ev.shape
    env = np.concatenate([a_pool, t_pool, np.asarray(context, f64).reshape(-1)])
    x = np.concatenate([np.repeat(af[:, None, :], MT, 1), np.repeat(tf[None, :, :], MA, 0), np.broadcast_to(env, (MA, MT, len(env)))], axis=2).reshape(MA * MT, -1)
    h = np.maximum(x @ w["w0"].astype(f64).T + w["b0"].astype(f64), 0)
    h = np.maximum(h @ w["w1"].astype(f64).T + w["b1"].astype(f64), 0)
    lg = (h @ w["w2"].astype(f64).T + w["b2"].astype(f64))[:, 0].reshape(MA, MT)
    return np.tanh(lg) * f64(f32(w["score_clamp"])) * (ev != 0), lg


load_weights = base.load_weights
as_state_dict = base.as_state_dict
