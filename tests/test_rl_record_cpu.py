"""The RL transition rings of the learned pair policies (MuavtaRlRings, muavta_rollout_record) without a device: the binding's layout against
the header, the frozen size of the C ABI, and the shapes / argument checks of `rl_record_shapes` / `rollout_rl_record` that need no device call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import policy_mlp_py as twin
from muavta_amd import native
from muavta_amd.batched import F, BatchedMultiUAVEnv
from muavta_amd.params import RL_RINGS, MuavtaRecord, MuavtaRlRings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "muavta.h")


def test_rl_rings_and_the_record_match_the_header_field_by_field(tmp_path):
    structs = {"MuavtaRlRings": MuavtaRlRings, "MuavtaRecord": MuavtaRecord}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "muavta.h"', 'int main(void) {']
    for name, st in structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for field, *_ in st._fields_:
            lines.append(f'  printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    lines += ['  printf("slots %d\\n", MUAVTA_RL_MAX_SLOTS);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, st in structs.items():
        assert int(got[name]) == C.sizeof(st), f"sizeof({name}): header {got[name]}, binding {C.sizeof(st)}"
        for field, *_ in st._fields_:
            assert int(got[f"{name}.{field}"]) == getattr(st, field).offset, f"{name}.{field}"
    assert int(got["slots"]) == BatchedMultiUAVEnv.RL_MAX_SLOTS == 4096
    # the new field is the record's LAST one, a pointer to the ring struct, and a zero-initialised record carries none
    assert MuavtaRecord._fields_[-1][0] == "rl" and MuavtaRecord.rl.offset + C.sizeof(C.c_void_p) == C.sizeof(MuavtaRecord)
    assert not MuavtaRecord().rl
    assert [f for f, *_ in MuavtaRlRings._fields_] == ["n_slots", "reserved"] + list(RL_RINGS)
    # every ring of the binding is a member of the header's struct, in the header's order
    text = open(HEADER).read()
    body = re.search(r"typedef struct MuavtaRlRings \{(.*?)\} MuavtaRlRings;", text, re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", body) == list(RL_RINGS)


def test_the_abi_gained_no_entry_point_and_no_field():
    assert len(native.EXPORTS) == 68 and len(set(native.EXPORTS)) == 68
    text = open(HEADER).read()
    protos = set(re.findall(r"^(?:int|const char\*)\s+(muavta_\w+)\(", text, re.M))
    assert protos == set(native.EXPORTS)
    enum = re.search(r"typedef enum \w*\s*\{(.*?)\}\s*MuavtaField;", text, re.S) or re.search(r"enum\s*\{([^}]*MUAVTA_F_AGENT_POS[^}]*)\}", text, re.S)
    names = re.findall(r"MUAVTA_F_(\w+)", enum.group(1))
    names = [n for n in dict.fromkeys(names) if n != "COUNT_"]
    assert len(names) == len(F) == 33 and names[-1] == "TOKEN_PADS" and F["TOKEN_PADS"] == 32


def _bare(kind_weights, n=8, pads=(32, 16), mode=6):
    """the object as the no-device tests of parse_pair_policy build it: no handle behind it"""
    env = BatchedMultiUAVEnv.__new__(BatchedMultiUAVEnv)
    env.n_envs, env.device_index, env._token_pads, env._alloc_mode = n, 0, pads, mode
    env._pair_policy = None if kind_weights is None else BatchedMultiUAVEnv.parse_pair_policy(twin.as_state_dict(twin.load_weights(*kind_weights)))
    env.h = C.c_void_p()
    return env


@pytest.mark.parametrize("kind,wname,dt,da,nc", [(twin.PAIR, "init2", 13, 12, None), (twin.PAIR, "init2_raw", 9, 11, None),
                                                 (twin.CONTEXT, "init2", 13, 12, 8), (twin.CONTEXT, "init2_raw", 9, 11, 1)])
def test_rl_record_shapes(kind, wname, dt, da, nc):
    G, N = 5, 8
    sh = _bare((kind, wname), N).rl_record_shapes(G)
    tok = {"task_feats": ((G, N, 32, dt), np.float32), "task_mask": ((G, N, 32), np.uint8), "agent_feats": ((G, N, 16, da), np.float32),
           "agent_mask": ((G, N, 16), np.uint8), "edge_valid": ((G, N, 16, 32), np.float32)}
    if nc is not None:
        tok["context"] = ((G, N, nc), np.float32)
    want = dict(tok)
    want.update({k: ((G, N, 16, 32), np.float32) for k in ("logits", "scores", "selected")})
    want.update({"s_wps_before": ((G, N), np.float64), "s_wps_after": ((G, N), np.float64)})
    want.update({"next_" + k: v for k, v in tok.items()})
    want.update({"done": ((G, N), np.uint8), "step": ((G, N), np.int32), "n_gates": ((N,), np.int32)})
    assert sh == want
    assert set(sh) | {"noise"} == set(RL_RINGS) if nc is not None else set(sh) | {"noise", "context", "next_context"} == set(RL_RINGS)


def test_argument_checks_raise_before_any_device_call():
    with pytest.raises(ValueError, match="no policy"):
        _bare(None).rl_record_shapes(4)
    with pytest.raises(ValueError, match="MLP-Coalition"):
        _bare((twin.COALITION, "init2")).rl_record_shapes(4)
    with pytest.raises(ValueError, match=r"\(32, 16\)"):
        _bare((twin.PAIR, "init2"), pads=(64, 48)).rl_record_shapes(4)
    env = _bare((twin.PAIR, "init2"))
    for bad in (0, -1, 4097):
        with pytest.raises(ValueError, match="n_slots"):
            env.rl_record_shapes(bad)
    assert env.rl_record_shapes(4096)["step"][0] == (4096, 8)
    import torch
    tdt = {np.float32: torch.float32, np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64}
    rings = {k: torch.zeros(shape, dtype=tdt[dt]) for k, (shape, dt) in env.rl_record_shapes(2).items()}
    seeds = np.arange(8, dtype=np.uint64)
    with pytest.raises(ValueError, match="mlp_pair"):
        _bare((twin.PAIR, "init2"), mode=0).rollout_rl_record(seeds, 10, 20, True, rings)
    with pytest.raises(ValueError, match="step"):
        env.rollout_rl_record(seeds, 10, 20, True, {k: v for k, v in rings.items() if k != "step"})
    with pytest.raises(ValueError, match="CUDA"):   # host tensors: refused at the first ring, nothing was launched (there is no handle)
        env.rollout_rl_record(seeds, 10, 20, True, rings)
    with pytest.raises(ValueError, match="lacks"):
        env.rollout_rl_record(seeds, 10, 20, True, {"step": rings["step"]})
