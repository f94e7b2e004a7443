"""What the wide-pad tests (test_wide_pads_cpu.py, test_gpu_wide_pads.py) share: the fixtures of tools/gen_golden_wide_pads.py, the params of
their cases and the replay of a recorded trace through the oracle's scored path."""
import glob
import os

import numpy as np

import policy_mlp_py as twin
from muavta_amd.params import params_for_case, params_from_config
from muavta_amd.scenarios import CASE_SPECS, TILES, WPS_ENV_FLAGS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MT, MA = 64, 48
URG_TRACES = sorted(glob.glob(os.path.join(GOLDEN, "urgpair48_trace_*.npz")))
URG_METRICS = sorted(glob.glob(os.path.join(GOLDEN, "urgpair48_metrics_*.npz")))
LEARNED = {"pair": (twin.PAIR, "mlppair48"), "context": (twin.CONTEXT, "mlpctx48")}
LEARNED_TRACES = {name: sorted(glob.glob(os.path.join(GOLDEN, f"{prefix}_trace_*.npz"))) for name, (_, prefix) in LEARNED.items()}
LEARNED_METRICS = {name: sorted(glob.glob(os.path.join(GOLDEN, f"{prefix}_metrics_*.npz"))) for name, (_, prefix) in LEARNED.items()}
ALL_LEARNED_TRACES = [(name, p) for name in LEARNED for p in LEARNED_TRACES[name]]
GATE_TRAINER, SC_EDGE_VALID_ONLY = 1, 1
METRIC_CASES = ("WPS_attn_OS24", "WPS_attn_L", "WPS_attn_XL")


def trace_id(v):
    return os.path.basename(v)[:-4] if isinstance(v, str) else None


def params_of(g, **tile):
    """the params of a fixture's case: a registry case, or the one WPS_burst64 was derived into with the task counts the file records"""
    case = str(g["case"])
    if case in CASE_SPECS:
        return params_for_case(case, **tile)
    base = case.rpartition("_T")[0]
    spec = dict(CASE_SPECS[base])
    spec["tasks"] = {"Att": int(g["tasks_att"]), "Rec": int(g["tasks_rec"]), "Hold": 0}
    ta, tt, th = TILES[base]
    return params_from_config(spec, dict(WPS_ENV_FLAGS), tile_agents=tile.get("tile_agents", ta), tile_tasks=tile.get("tile_tasks", tt), tile_threats=tile.get("tile_threats", th))


def token_kind(g, w=None):
    """MUAVTA_TOK_PAIR / _PAIR_RAW of a trace (an Urgency-Pair trace: plain pair tokens)"""
    return 1 if (w is not None and w["raw_features"]) else 0


def actions_at(g, t):
    """(agent id, open index) rows of step t, ascending agent id; the Urgency-Pair traces carry the task id as a third column"""
    a = g["actions"][g["actions"][:, 0] == t]
    a = a[:, [1, a.shape[1] - 1]]
    return a[np.argsort(a[:, 0], kind="stable")]


def d_ref(g):
    """the reference's own float32 deviation from a float64 evaluation of the same net on the same tokens, on this trace"""
    ev = g["ev"] != 0
    return float(np.abs(g["scores"].astype(np.float64) - g["scores64"])[ev].max())


def weights_of(name, g):
    return twin.load_weights(LEARNED[name][0], str(g["weights"]))
