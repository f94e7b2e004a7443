"""Host twin of the device's MLP-Pair forward pass (csrc/sim/policy.inc) — the arithmetic contract of DESIGN.md §7, restated with numpy.

Exact up to the logits: every Linear output is ONE k-ascending float32 fma chain that starts from the bias,

    acc = b[n];  for k in 0..K-1:  acc = fma(W[n][k], x[k], acc)          (one rounding per step)

with x = the agent row's features followed by the task row's (the reference's `cat`), ReLU = (acc > 0 ? acc : 0) between the
layers.  `fma32` is a correctly rounded float32 fma: `math.fma` does not exist before Python 3.13 and is scalar, so the product is
formed in float64 (exact: 24 + 24 significant bits), added to the addend with an error-free TwoSum, and the one case in which rounding
the float64 sum to float32 could differ from rounding the exact sum — the float64 sum sits exactly half way between two float32
neighbours — is decided by the sign of the TwoSum error.  Scores are `np.tanh` in float32 times score_clamp: the device's tanhf may
differ from it in the last bits, so scores are compared with a tolerance and logits bit for bit.
"""
from __future__ import annotations

import numpy as np

f32, f64 = np.float32, np.float64


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


def pair_logits(w, x):
    """x [P, K] float32 (agent features then task features) -> logits [P] float32."""
    h = relu(linear(w["w0"], w["b0"], x))
    h = relu(linear(w["w1"], w["b1"], h))
    return linear(w["w2"], w["b2"], h)[:, 0]


def forward(w, agent_feats, task_feats, edge_valid):
    """Token tensors of ONE env ([MA, Da], [MT, Dt], [MA, MT]) -> (scores, logits) [MA, MT] float32; 0 where edge_valid is 0 (those
    pairs are not evaluated, as on the device)."""
    af, tf, ev = np.asarray(agent_feats, f32), np.asarray(task_feats, f32), np.asarray(edge_valid)
    ii, jj = np.nonzero(ev != 0)
    logits = np.zeros(ev.shape, f32)
    scores = np.zeros(ev.shape, f32)
    if len(ii):
        lg = pair_logits(w, np.concatenate([af[ii], tf[jj]], axis=1))
        logits[ii, jj] = lg
        scores[ii, jj] = (np.tanh(lg) * f32(w["score_clamp"])).astype(f32)
    return scores, logits


def forward64(w, agent_feats, task_feats, edge_valid):
    """The same net in float64 (numpy matmul): the yardstick `scores64` of the fixtures."""
    af, tf, ev = np.asarray(agent_feats, f64), np.asarray(task_feats, f64), np.asarray(edge_valid)
    MA, MT = ev.shape
    x = np.concatenate([np.repeat(af[:, None, :], MT, 1), np.repeat(tf[None, :, :], MA, 0)], axis=2).reshape(MA * MT, -1)
    h = np.maximum(x @ w["w0"].astype(f64).T + w["b0"].astype(f64), 0)
    h = np.maximum(h @ w["w1"].astype(f64).T + w["b1"].astype(f64), 0)
    lg = (h @ w["w2"].astype(f64).T + w["b2"].astype(f64))[:, 0].reshape(MA, MT)
    return np.tanh(lg) * f64(f32(w["score_clamp"])) * (ev != 0), lg


def load_weights(path):
    z = np.load(path)
    w = {k: np.ascontiguousarray(z[k], f32) for k in ("w0", "b0", "w1", "b1", "w2", "b2")}
    w["raw_features"] = bool(z["raw_features"])
    w["score_clamp"] = float(z["score_clamp"])
    return w


def as_state_dict(w):
    """the mapping `BatchedMultiUAVEnv.set_pair_policy` takes"""
    d = {f"pair_mlp.{i}.{k}": w[f"{n}{j}"] for j, i in enumerate((0, 2, 4)) for k, n in (("weight", "w"), ("bias", "b"))}
    d["raw_features"] = w["raw_features"]
    d["score_clamp"] = w["score_clamp"]
    return d
