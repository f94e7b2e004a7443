"""Host twin of the device's learned-policy forward passes (csrc/sim/policy.inc) — the arithmetic contract of DESIGN.md §7 and §7.1,
restated with numpy.  One chain, one descriptor per kind (`PAIR`, `CONTEXT`, `COALITION`: the test-side mirror of PolPair / PolContextPair /
PolCoalition in csrc/muavta_device.h), and `forward` / `forward_batch` / `forward64` written once over the descriptor.

Exact up to the logits: every Linear output is ONE k-ascending float32 fma chain that starts from the bias,

    acc = b[n];  for k in 0..K-1:  acc = fma(W[n][k], x[k], acc)          (one rounding per step)

with ReLU = (acc > 0 ? acc : 0) between the three layers.  `fma32` is a correctly rounded float32 fma: `math.fma` does not exist before
Python 3.13 and is scalar, so the product is formed in float64 (exact: 24 + 24 significant bits), added to the addend with an error-free
TwoSum, and the one case in which rounding the float64 sum to float32 could differ from rounding the exact sum — the float64 sum sits
exactly half way between two float32 neighbours — is decided by the sign of the TwoSum error.

What the kinds differ in:

  input row   MLP-Pair, MLP-Coalition: the agent row's features followed by the task row's (the reference's `cat`).
              MLP-ContextPair: a_pool, t_pool, context, the agent row, the task row — in this order, ascending within each.  The state_dict's
              columns come in the reference's cat order (agent, task, a_pool, t_pool, context): `device_columns` is the permutation the
              packing step applies to layer 1's weights.  A pool is, for each feature column d: s = 0.0f; s = s + x[row][d] in float32 over
              the rows whose mask is 0 (non-pad), ascending row; pool[d] = s / float32(max(count, 1)), one correctly rounded float32
              division (a_pool: the 16 agent rows, t_pool: the 32 task rows).  The context is an input: what muavta_context(kind, 32)
              returns (pinned bit-exact against build_context_summary elsewhere).
  cells       MLP-Pair, MLP-ContextPair: the pairs whose edge_valid is 1.  MLP-Coalition: those that are not pad either (both masks).
              The other cells are not evaluated, as on the device, and report 0.
  score       MLP-Pair, MLP-ContextPair: `np.tanh` in float32 times score_clamp.  MLP-Coalition: 1 / (1 + exp(-clip(logit, -20, 20))),
              AttentionEscort.act's formula, with numpy's float32 exp and division.  The device's tanhf / expf may differ from numpy's in
              the last bits, so scores are compared with a tolerance and logits bit for bit.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Callable

import numpy as np

f32, f64 = np.float32, np.float64
KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fma32(a, b, c):
    """round_to_float32(a * b + c) for float32 arrays (broadcast), rounded once."""
    a, b, c = np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32)
    p = a.astype(f64) * b.astype(f64)          # exact
    c64 = np.broadcast_to(c.astype(f64), np.broadcast(p, c).shape)
    p = np.broadcast_to(p, c64.shape)
    s = p + c64                                # TwoSum: s + e == p + c exactly
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)
    r = s.astype(f32)
    rd = r.astype(f64)
    off = rd != s                              # s is not a float32: it lies strictly between two neighbours
    if np.any(off & (e != 0)):
        lo = np.where(rd < s, r, np.nextafter(r, f32(-np.inf)))
        hi = np.where(rd < s, np.nextafter(r, f32(np.inf)), r)
        tie = off & (s == (lo.astype(f64) + hi.astype(f64)) * 0.5) & np.isfinite(hi) & np.isfinite(lo)
        r = np.where(tie & (e > 0), hi, np.where(tie & (e < 0), lo, r))
    return r.astype(f32)


def linear(W, b, x):
    """x [P, K] -> [P, N]: the k-ascending fma chain from the bias, every (pair, output) element by itself."""
    W, b, x = np.asarray(W, f32), np.asarray(b, f32), np.asarray(x, f32)
    acc = np.broadcast_to(b[None, :], (x.shape[0], W.shape[0])).astype(f32)
    for k in range(W.shape[1]):
        acc = fma32(W[None, :, k], x[:, k, None], acc)
    return acc


def relu(v):
    return np.where(v > 0, v, f32(0)).astype(f32)


def sigmoid32(logits):
    """AttentionEscort.act's formula in float32"""
    lg = np.clip(np.asarray(logits, f32), f32(-20), f32(20))
    return (f32(1) / (f32(1) + np.exp(-lg, dtype=f32))).astype(f32)


def sigmoid64(logits):
    return 1.0 / (1.0 + np.exp(-np.clip(np.asarray(logits, f64), -20.0, 20.0)))


# ---------------------------------------------------------------- the context kind's input prefix
def dims(raw):
    """MLP-ContextPair: (agent features, task features, context floats)"""
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


# ---------------------------------------------------------------- the kinds
@dataclass(frozen=True)
class Kind:
    name: str            # 'kind' of BatchedMultiUAVEnv.parse_pair_policy
    fixtures: str        # tests/golden/<fixtures>{weights,trace,metrics}_*.npz
    max_tasks: int       # token grid: max_agents x max_tasks
    pad_masks: bool      # cells: edge_valid only, or edge_valid and both pad masks
    context: bool        # layer 1 reads a_pool, t_pool, context ahead of the pair's rows
    score: Callable      # (w, logits float32) -> scores float32
    score64: Callable    # the same in float64
    max_agents: int = 16


def _tanh_clamp(w, lg):
    return (np.tanh(lg) * f32(w["score_clamp"])).astype(f32)


def _tanh_clamp64(w, lg):
    return np.tanh(lg) * f64(f32(w["score_clamp"]))


PAIR = Kind("pair", "mlppair_", 32, False, False, _tanh_clamp, _tanh_clamp64)
CONTEXT = Kind("context", "mlpctx_", 32, False, True, _tanh_clamp, _tanh_clamp64)
COALITION = Kind("coalition", "mlpcoal_", 48, True, False, lambda w, lg: sigmoid32(lg), lambda w, lg: sigmoid64(lg))
KINDS = {k.name: k for k in (PAIR, CONTEXT, COALITION)}

TRACE_NAMES = {"agent_feats": "af", "task_feats": "tf", "edge_valid": "ev", "agent_mask": "amask", "task_mask": "tmask", "context": "ctx"}


def trace_tokens(g, k):
    """plan k of a recorded trace as the token dict of one env"""
    return {name: g[short][k] for name, short in TRACE_NAMES.items() if short in g}


def cells(kind, tok):
    """the pairs that are evaluated: bool [..., MA, MT] of one env's token dict or a batch's"""
    ok = np.asarray(tok["edge_valid"]) != 0
    if kind.pad_masks:
        ok = ok & (np.asarray(tok["agent_mask"]) == 0)[..., :, None] & (np.asarray(tok["task_mask"]) == 0)[..., None, :]
    return ok


def logits(kind, w, x):
    """x [P, K] float32 in device order -> logits [P] float32"""
    w0 = np.ascontiguousarray(w["w0"][:, device_columns(w["w0"].shape[1] == 41)]) if kind.context else w["w0"]
    h = relu(linear(w0, w["b0"], x))
    h = relu(linear(w["w1"], w["b1"], h))
    return linear(w["w2"], w["b2"], h)[:, 0]


def forward_batch(kind, w, tok):
    """The token dict of N envs (`BatchedMultiUAVEnv.tokens`; the context kind: plus 'context', what `.context` returns) ->
    (scores, logits) [N, MA, MT] float32, 0 where the cell is not evaluated; one chain evaluation for every cell of the batch."""
    af, tf = np.asarray(tok["agent_feats"], f32), np.asarray(tok["task_feats"], f32)
    ok = cells(kind, tok)
    nn, ii, jj = np.nonzero(ok)
    lgs = np.zeros(ok.shape, f32)
    scores = np.zeros(ok.shape, f32)
    if len(nn):
        x = np.concatenate([af[nn, ii], tf[nn, jj]], axis=1)
        if kind.context:
            pre = {n: prefix(af[n], tok["agent_mask"][n], tf[n], tok["task_mask"][n], tok["context"][n]) for n in np.unique(nn)}
            x = np.concatenate([np.stack([pre[n] for n in nn]), x], axis=1).astype(f32)
        lg = logits(kind, w, x)
        lgs[nn, ii, jj] = lg
        scores[nn, ii, jj] = kind.score(w, lg)
    return scores, lgs


def forward(kind, w, tok):
    """Token dict of ONE env ([MA, Da], [MT, Dt], [MA, MT], ...) -> (scores, logits) [MA, MT] float32"""
    s, lg = forward_batch(kind, w, {k: np.asarray(v)[None] for k, v in tok.items()})
    return s[0], lg[0]


def forward64(kind, w, tok):
    """The same net in float64 (numpy matmul; the context kind: pooling included) on the float32 tokens of ONE env, in the reference's
    column order: the yardstick `scores64` of the fixtures.  -> (scores, logits) [MA, MT] float64"""
    af, tf = np.asarray(tok["agent_feats"], f64), np.asarray(tok["task_feats"], f64)
    ok = cells(kind, tok)
    MA, MT = ok.shape
    cols = [np.repeat(af[:, None, :], MT, 1), np.repeat(tf[None, :, :], MA, 0)]
    if kind.context:
        am, tm = (np.asarray(tok["agent_mask"]) == 0).astype(f64)[:, None], (np.asarray(tok["task_mask"]) == 0).astype(f64)[:, None]
        a_pool = (af * am).sum(0) / max(am.sum(), 1.0)
        t_pool = (tf * tm).sum(0) / max(tm.sum(), 1.0)
        env = np.concatenate([a_pool, t_pool, np.asarray(tok["context"], f64).reshape(-1)])
        cols.append(np.broadcast_to(env, (MA, MT, len(env))))
    x = np.concatenate(cols, axis=2).reshape(MA * MT, -1)
    h = np.maximum(x @ w["w0"].astype(f64).T + w["b0"].astype(f64), 0)
    h = np.maximum(h @ w["w1"].astype(f64).T + w["b1"].astype(f64), 0)
    lg = (h @ w["w2"].astype(f64).T + w["b2"].astype(f64))[:, 0].reshape(MA, MT)
    return kind.score64(w, lg) * ok, lg


# ---------------------------------------------------------------- weights
def weight_sets(kind):
    return sorted(f[len(kind.fixtures) + len("weights_"):-4] for f in os.listdir(GOLDEN) if f.startswith(kind.fixtures + "weights_"))


def load_weights(kind, name):
    """weight set `name` of the kind's fixtures; a file with a 'base' entry holds layer 3 only, over that other set"""
    z = np.load(os.path.join(GOLDEN, f"{kind.fixtures}weights_{name}.npz"))
    if "base" in z.files:
        w = load_weights(kind, str(z["base"]))
        w["w2"], w["b2"] = np.ascontiguousarray(z["w2"], f32), np.ascontiguousarray(z["b2"], f32)
        return w
    w = {k: np.ascontiguousarray(z[k], f32) for k in KEYS}
    if "raw_features" in z.files:
        w["raw_features"] = bool(z["raw_features"])
        w["score_clamp"] = float(z["score_clamp"])
    return w


def as_state_dict(w):
    """the mapping `BatchedMultiUAVEnv.set_pair_policy` takes (layer 1's width tells the kinds apart)"""
    d = {f"pair_mlp.{i}.{k}": w[f"{n}{j}"] for j, i in enumerate((0, 2, 4)) for k, n in (("weight", "w"), ("bias", "b"))}
    d.update({k: w[k] for k in ("raw_features", "score_clamp") if k in w})
    return d


def as_checkpoint(w):
    """what AttentionEscort.save writes for an MLP-Coalition (tensors as arrays)"""
    return {"state_dict": as_state_dict(w), "use_attention": False, "max_tasks": COALITION.max_tasks, "max_agents": COALITION.max_agents, "d_model": 128,
            "nhead": 4, "n_layers": 3, "lr": 3e-4, "version": 2}
