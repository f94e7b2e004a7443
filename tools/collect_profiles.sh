#!/bin/bash
# Runs ON THE GPU BOX (via gpurun): for each BASELINE config's tile, a rocprofv3 kernel trace and the PMC passes the HBM
# guide prescribes (FETCH_SIZE and WRITE_SIZE cannot share a pass), each with --kernel-trace only and the program directly
# after `--`.  Output under gpurun_out/prof_<tag>/<case>/; tools/summarize_profiles.py turns it into profiles/<tag>_*.
# Every pass runs under its own time limit and the first pass that fails ends the collection: nothing more is started on
# a GPU after a run on it went wrong.  MUAVTA_SO (muavta_amd/native.py) selects another build of the library, e.g. the
# parent commit's for a "before" collection.
set -u
TAG=${1:-r04}
CASES=${2:-"WPS_hard_x2:4096 WPS_escort24:4096 WPS_burst64:1024"}
LIMIT=${PASS_SECONDS:-150}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
pass() {  # name, stdout file, command ...
  local name=$1 out=$2; shift 2
  timeout -k 10 "$LIMIT" "$@" > "$out" 2> "$OUT/$name.err"
  local rc=$?
  if [ $rc -ne 0 ]; then echo "$c: pass $name failed with status $rc; collection stopped"; tail -5 "$OUT/$name.err"; exit $rc; fi
}
for ce in $CASES; do
  c=${ce%%:*}; n=${ce##*:}
  OUT=gpurun_out/prof_$TAG/$c
  mkdir -p "$OUT"
  ARGS="bench.py --case $c --envs $n --no-cpu-baseline --no-extras"
  PARGS="$ARGS --lanes 1"  # counter passes: one state lane, launches in order (per-dispatch counters of overlapping launches are not separable)
  pass kt "$OUT/bench_kt.json" rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/kt" -- python3 $ARGS --steps 10 --warmup 2
  pass fetch /dev/null rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d "$OUT/fetch" -- python3 $PARGS --steps 4 --warmup 1
  pass write /dev/null rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d "$OUT/write" -- python3 $PARGS --steps 4 --warmup 1
  pass sq1 /dev/null rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAIT_ANY SQ_WAIT_INST_ANY --output-format csv -d "$OUT/sq1" -- python3 $PARGS --steps 4 --warmup 1
  pass sq2 /dev/null rocprofv3 --kernel-trace --pmc SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_SCA SQ_INSTS_SMEM SQ_INSTS_VMEM_WR SQ_INSTS_VMEM_RD SQ_INSTS_BRANCH --output-format csv -d "$OUT/sq2" -- python3 $PARGS --steps 4 --warmup 1
  pass sq3 /dev/null rocprofv3 --kernel-trace --pmc SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_IFETCH SQ_INST_CYCLES_SALU SQ_INST_CYCLES_SMEM SQ_INST_CYCLES_VMEM SQ_ACTIVE_INST_VMEM --output-format csv -d "$OUT/sq3" -- python3 $PARGS --steps 4 --warmup 1
  pass sq4 /dev/null rocprofv3 --kernel-trace --pmc SQ_THREAD_CYCLES_VALU SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_TRANS_F64 SQ_INSTS_VALU_INT32 --output-format csv -d "$OUT/sq4" -- python3 $PARGS --steps 4 --warmup 1
  pass bench "$OUT/bench.json" python3 $ARGS
  echo "$c done: $(cut -c1-200 "$OUT/bench.json")"
done
