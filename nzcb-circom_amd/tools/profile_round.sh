#!/bin/bash
# One profiling call for profiles/ (on the GPU box, from the repo root), into the directory
# named by PROFILE_OUT, then `python3 nzcb-circom_amd/tools/collect_profiles.py --prefix rN
# --src <that directory>` here:
#   prof/       rocprofv3 --kernel-trace --stats of the default bench.py --full run
#   pmc_fetch/  FETCH_SIZE, pmc_write/ WRITE_SIZE (separate passes, bench.py --full --steps 8)
#   pmcv/       SQ_INSTS_VALU SQ_WAVES by kernel, one lane (where the VALU goes per proof)
#   pmcA/ pmcB/ the isolated accumulation's SQ and GRBM counters (tools/acc_probe.py)
#   lane1/      kernel + roctx marker trace of single-lane proofs (tools/phase_kernels.py)
#   microbench.log  MSM and NTT 2^18..2^24 (configs[1])
# The bench runs pass --full: the trace and the PMC passes read the isolated accumulation
# probe (the run's last launches) and the line's roofline; the single-lane runs count the
# latency proofs. Each step has its own time limit; the first failure ends the call.
set -o pipefail
O=${PROFILE_OUT:?set PROFILE_OUT to the directory the profiles go to (relative to the repo root)}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
mkdir -p $O
rm -rf $O/prof $O/pmc_fetch $O/pmc_write $O/pmcv $O/pmcA $O/pmcB $O/lane1
step() { echo "== $1 $(date +%T)"; }
step trace
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $O/prof -o run --output-format csv \
  -- python3 bench.py --full > $O/prof_bench.log 2>&1 || exit $?
step fetch
timeout -s KILL 300 rocprofv3 --pmc FETCH_SIZE -d $O/pmc_fetch -o run --output-format csv \
  -- python3 bench.py --full --no-cpu-baseline --steps 8 > $O/pmc_fetch.log 2>&1 || exit $?
step write
timeout -s KILL 300 rocprofv3 --pmc WRITE_SIZE -d $O/pmc_write -o run --output-format csv \
  -- python3 bench.py --full --no-cpu-baseline --steps 8 > $O/pmc_write.log 2>&1 || exit $?
step valu
timeout -s KILL 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES -d $O/pmcv -o run --output-format csv \
  -- python3 bench.py --full --lanes 1 --steps 4 --warmup 1 --no-cpu-baseline --no-probe > $O/pmcv.log 2>&1 || exit $?
step accA
timeout -s KILL 120 rocprofv3 --pmc SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_WAIT_ANY \
  SQ_WAIT_INST_ANY SQ_WAVES SQ_WAVE_CYCLES -d $O/pmcA -o run --output-format csv \
  -- python3 nzcb-circom_amd/tools/acc_probe.py > $O/pmcA.log 2>&1 || exit $?
step accB
timeout -s KILL 120 rocprofv3 --pmc GRBM_COUNT GRBM_GUI_ACTIVE SQ_ACTIVE_INST_MISC SQ_INSTS_SALU SQ_INSTS_VMEM_RD \
  SQ_INST_CYCLES_VMEM_RD -d $O/pmcB -o run --output-format csv \
  -- python3 nzcb-circom_amd/tools/acc_probe.py > $O/pmcB.log 2>&1 || exit $?
step lane1
timeout -k 10 300 rocprofv3 --kernel-trace --marker-trace -d $O/lane1 -o run --output-format csv \
  -- python3 bench.py --full --lanes 1 --steps 6 --warmup 2 --no-cpu-baseline --no-probe > $O/lane1.log 2>&1 \
  || exit $?
step microbench
timeout -k 10 300 python3 -u nzcb-circom_amd/tools/microbench.py > $O/microbench.log 2>&1 || exit $?
step done
echo profile-ok
