"""Where csrc/muavta_state.h puts Task.initTime / doneTime on each tile (TaskTimes, Tile::TIMES_LDS), read from a host program that includes
the header: the 16-agent tile keeps them in the LDS record and stays under the 10,240 B that 16 envs per CU allow, the other tiles keep them
in the HBM record exactly where they were, and the size of a muavta_get_state record (the sum of both) is what it was."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-uav-ta-gym-env_amd", "csrc")

SRC = r"""
#include <cstdio>
#include <cstddef>
#include <type_traits>
#include "muavta_state.h"
template <class TL> void show(int n) {
  typedef EnvState<TL> S; typedef EnvCold<TL> C;
  const bool in_state = std::is_base_of<TaskTimes<TL::T, true>, S>::value, in_cold = std::is_base_of<TaskTimes<TL::T, true>, C>::value;
  size_t off_init, off_dtime, off_after;
  if constexpr (TL::TIMES_LDS) { off_init = offsetof(S, t_init); off_dtime = offsetof(S, t_dtime); off_after = offsetof(S, a_px); }
  else { off_init = offsetof(C, t_init); off_dtime = offsetof(C, t_dtime); off_after = offsetof(C, a_qtime); }
  printf("%d %d %d %d %zu %zu %zu %zu %zu %zu %zu\n", n, (int)TL::TIMES_LDS, (int)in_state, (int)in_cold, sizeof(S), sizeof(C), off_init, off_dtime, off_after,
         offsetof(C, t_cur), offsetof(C, t_alloc));
}
int main() { show<Tile16>(16); show<Tile24>(24); show<Tile64>(64); return 0; }
"""
# sizeof(EnvState) + sizeof(EnvCold) per tile before the two arrays could move (muavta_dims' state_bytes: 12.4 / 16.8 / 43.8 KB)
RECORD_BYTES = {16: 6400 + 5952, 24: 7520 + 9296, 64: 23168 + 20672}
COLD_BYTES = {24: 9296, 64: 20672}


def _layout(tmp_path, *defines):
    src, exe = tmp_path / "layout.cpp", tmp_path / ("layout" + "".join(defines).replace("=", "_"))
    src.write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-w", *defines, "-I", CSRC, "-o", str(exe), str(src)])
    rows = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        w = [int(x) for x in line.split()]
        rows[w[0]] = dict(zip(("flag", "in_state", "in_cold", "state", "cold", "init", "dtime", "after", "t_cur", "t_alloc"), w[1:]))
    return rows


def test_task_times_live_in_lds_on_the_16_agent_tile_only(tmp_path):
    rows = _layout(tmp_path)
    assert (rows[16]["flag"], rows[16]["in_state"], rows[16]["in_cold"]) == (1, 1, 0)
    for t in (24, 64):
        assert (rows[t]["flag"], rows[t]["in_state"], rows[t]["in_cold"]) == (0, 0, 1)
        assert rows[t]["cold"] == COLD_BYTES[t]
    T = {16: 40, 24: 48, 64: 128}
    for t, r in rows.items():
        assert r["state"] + r["cold"] == RECORD_BYTES[t], f"tile {t}: muavta_get_state record size"
        assert r["state"] % 16 == 0 and r["cold"] % 16 == 0
        assert r["dtime"] - r["init"] == 8 * T[t] and r["after"] - r["dtime"] == 8 * T[t], f"tile {t}: the two arrays are contiguous"
        assert r["t_alloc"] - r["t_cur"] == 48 * T[t]
        if not r["flag"]:
            assert r["init"] == r["t_alloc"] + 48 * T[t], f"tile {t}: the times follow allocatedReqs in the HBM record, as they always have"
    assert rows[16]["state"] == 6400 + 640


def test_knob_off_is_the_record_as_it_was(tmp_path):
    rows = _layout(tmp_path, "-DMUAVTA_TIMES_LDS=0")
    assert (rows[16]["flag"], rows[16]["in_state"], rows[16]["in_cold"]) == (0, 0, 1)
    assert (rows[16]["state"], rows[16]["cold"]) == (6400, 5952)
    assert rows[16]["init"] == rows[16]["t_alloc"] + 48 * 40

