#!/bin/bash
# The rocprofv3 runs behind profiles/r02_*: run on the MI355X box from anywhere (`bash bench/tools/collect_profiles.sh OUT`),
# outputs land under the directory OUT and are summarised into profiles/ by the python steps at the bottom (run those where the repo is).
# PMC counters are collected in their own passes (no trace domains), as MI355X_MICROARCH.md prescribes.
O=$(realpath -m "${1:?usage: collect_profiles.sh OUT}")
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
# 1. kernel durations of the bench command itself (3 streams) and of the single-stream variant
rocprofv3 --kernel-trace --stats --output-format csv -d $O/r02_stats -o bench -- python $R/bench.py --full --no-cpu-baseline --no-create-proof > $O/r02_stats_bench.json 2>/dev/null
rocprofv3 --kernel-trace --stats --output-format csv -d $O/r02_stats1 -o bench1 -- python $R/bench.py --full --streams 1 --steps 40 --no-cpu-baseline --no-create-proof > $O/r02_stats1_bench.json 2>/dev/null
# 2. HBM traffic: FETCH_SIZE and WRITE_SIZE in separate passes over the minimal workload (timed commits + NTT leg)
rocprofv3 --pmc FETCH_SIZE -d $O/r02_pmc_f -o f --output-format csv -- python $R/bench.py --full --steps 3 --warmup 1 --prewarm-ms 0 --minimal --no-cpu-baseline --streams 1 > /dev/null 2>&1
rocprofv3 --pmc WRITE_SIZE -d $O/r02_pmc_w -o w --output-format csv -- python $R/bench.py --full --steps 3 --warmup 1 --prewarm-ms 0 --minimal --no-cpu-baseline --streams 1 > /dev/null 2>&1
# 3. issue / wait shares of a wave's cycles (SQ counters, one pass)
C="SQ_WAVE_CYCLES SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE"
rocprofv3 --pmc $C -d $O/r02_sq_ntt -o n --output-format csv -- python $R/bench/tools/ntt_only.py 22 > /dev/null 2>&1
rocprofv3 --pmc $C -d $O/r02_sq_msm -o m --output-format csv -- python $R/bench.py --full --steps 3 --warmup 1 --prewarm-ms 0 --minimal --no-cpu-baseline --streams 1 > /dev/null 2>&1
# afterwards, in the repo:
#   python bench/pmc_summary.py OUT/r02_pmc_f/f_counter_collection.csv OUT/r02_pmc_w/w_counter_collection.csv > profiles/r02_pmc_traffic.json
#   python bench/tools/trace_union.py OUT/r02_stats/bench_kernel_trace.csv  > profiles/r02_accumulate_union_3streams.json
#   python bench/tools/trace_union.py OUT/r02_stats1/bench1_kernel_trace.csv > profiles/r02_accumulate_union_1stream.json
#   cp OUT/r02_stats/bench_kernel_stats.csv profiles/r02_kernel_stats_3streams.csv   (and the 1-stream one)
