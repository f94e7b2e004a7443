"""Host twin of the device's MLP-Coalition forward pass (csrc/sim/policy.inc, CoalitionLayout) — the arithmetic contract of DESIGN.md §7.1,
restated with numpy over tests/pair_mlp_py.fma32.

    logits = pair_mlp(cat([agent_feats[i], task_feats[j]]))       Linear(38, 256) - ReLU - Linear(256, 256) - ReLU - Linear(256, 1)
    score  = 1 / (1 + exp(-clip(logit, -20, 20)))                 float32, on the pairs that are not pad and whose edge_valid is 1

Exact up to the logits: every Linear output is ONE k-ascending float32 fma chain from the bias (layer 1 over the agent row's 16 features,
then the task row's 22).  The score is numpy's float32 exp and division: the device's expf may differ in the last bits, so scores are
compared with a tolerance and logits bit for bit.  Pad pairs and pairs whose edge_valid is 0 are not evaluated and report 0.
"""
from __future__ import annotations

import numpy as np

from pair_mlp_py import f32, f64, pair_logits

KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")
MT, MA, DT, DA, HID = 48, 16, 22, 16, 256


def sigmoid32(logits):
    """AttentionEscort.act's formula in float32"""
    lg = np.clip(np.asarray(logits, f32), f32(-20), f32(20))
    return (f32(1) / (f32(1) + np.exp(-lg, dtype=f32))).astype(f32)


def sigmoid64(logits):
    return 1.0 / (1.0 + np.exp(-np.clip(np.asarray(logits, f64), -20.0, 20.0)))


def valid_pairs(agent_mask, task_mask, edge_valid):
    return (np.asarray(edge_valid) != 0) & (np.asarray(agent_mask) == 0)[:, None] & (np.asarray(task_mask) == 0)[None, :]


def forward32(w, agent_feats, agent_mask, task_feats, task_mask, edge_valid):
    """Token tensors of ONE env ([16, 16], [16], [48, 22], [48], [16, 48]) -> (scores, logits) [16, 48] float32"""
    af, tf = np.asarray(agent_feats, f32), np.asarray(task_feats, f32)
    ok = valid_pairs(agent_mask, task_mask, edge_valid)
    ii, jj = np.nonzero(ok)
    logits = np.zeros(ok.shape, f32)
    scores = np.zeros(ok.shape, f32)
    if len(ii):
        lg = pair_logits(w, np.concatenate([af[ii], tf[jj]], axis=1))
        logits[ii, jj] = lg
        scores[ii, jj] = sigmoid32(lg)
    return scores, logits


def forward64(w, agent_feats, agent_mask, task_feats, task_mask, edge_valid):
    """The same net in float64 (numpy matmul) on the float32 tokens: the yardstick `scores64` of the fixtures -> (scores, logits)"""
    af, tf = np.asarray(agent_feats, f64), np.asarray(task_feats, f64)
    ok = valid_pairs(agent_mask, task_mask, edge_valid)
    A, T = ok.shape
    x = np.concatenate([np.repeat(af[:, None, :], T, 1), np.repeat(tf[None, :, :], A, 0)], axis=2).reshape(A * T, -1)
    h = np.maximum(x @ w["w0"].astype(f64).T + w["b0"].astype(f64), 0)
    h = np.maximum(h @ w["w1"].astype(f64).T + w["b1"].astype(f64), 0)
    lg = (h @ w["w2"].astype(f64).T + w["b2"].astype(f64))[:, 0].reshape(A, T)
    return sigmoid64(lg) * ok, lg


def forward_batch(w, tok):
    """`BatchedMultiUAVEnv.tokens("escort", 48, 16)` of N envs -> (scores, logits) [N, 16, 48]; every valid pair of the batch in one call"""
    af, tf = np.asarray(tok["agent_feats"], f32), np.asarray(tok["task_feats"], f32)
    ok = (np.asarray(tok["edge_valid"]) != 0) & (np.asarray(tok["agent_mask"]) == 0)[:, :, None] & (np.asarray(tok["task_mask"]) == 0)[:, None, :]
    nn, ii, jj = np.nonzero(ok)
    logits = np.zeros(ok.shape, f32)
    scores = np.zeros(ok.shape, f32)
    if len(nn):
        lg = pair_logits(w, np.concatenate([af[nn, ii], tf[nn, jj]], axis=1))
        logits[nn, ii, jj] = lg
        scores[nn, ii, jj] = sigmoid32(lg)
    return scores, logits


def load_weights(path):
    z = np.load(path)
    return {k: np.ascontiguousarray(z[k], f32) for k in KEYS}


def as_state_dict(w):
    """the mapping `BatchedMultiUAVEnv.set_pair_policy` takes (pair_mlp.0.weight [256, 38] marks it as an MLP-Coalition)"""
    return {f"pair_mlp.{i}.{k}": w[f"{n}{j}"] for j, i in enumerate((0, 2, 4)) for k, n in (("weight", "w"), ("bias", "b"))}


def as_checkpoint(w):
    """what AttentionEscort.save writes for an MLP-Coalition (tensors as arrays)"""
    return {"state_dict": as_state_dict(w), "use_attention": False, "max_tasks": MT, "max_agents": MA, "d_model": 128, "nhead": 4,
            "n_layers": 3, "lr": 3e-4, "version": 2}
