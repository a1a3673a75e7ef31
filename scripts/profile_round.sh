#!/bin/bash
# run on the GPU box (through gpurun): the three rocprofv3 passes scripts/make_profiles.py reads, then the bench lines of the round
# (official C2 line, fp32 line, configs[2] and configs[4] lines, C3 kernel stats).  Counters never share a run with traces other than the kernel trace.
# (everything is written under $PROFILE_OUT, default <repo>/profile_out; make_profiles.py reads it from there)
set -e
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${PROFILE_OUT:-$R/profile_out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_stats $OUT/prof_fetch $OUT/prof_write $OUT/prof_c3
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_stats -o s -- python3 $R/bench.py --full --no-cpu-baseline --no-secondary > $OUT/prof_stats.log 2>&1
rm -f $OUT/prof_stats/*/*kernel_trace.csv $OUT/prof_stats/*kernel_trace.csv
timeout -k 10 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/prof_fetch -o f -- python3 $R/bench.py --no-graph --steps 3 --warmup 1 --no-cpu-baseline --no-roofline --no-secondary > $OUT/prof_fetch.log 2>&1
rm -f $OUT/prof_fetch/*/*kernel_trace.csv $OUT/prof_fetch/*kernel_trace.csv
timeout -k 10 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/prof_write -o w -- python3 $R/bench.py --no-graph --steps 3 --warmup 1 --no-cpu-baseline --no-roofline --no-secondary > $OUT/prof_write.log 2>&1
rm -f $OUT/prof_write/*/*kernel_trace.csv $OUT/prof_write/*kernel_trace.csv
# matrix-core utilisation (north_star: "choices evidenced by rocprof HBM GB/s and MFMA utilisation"): SQ / GRBM counters only, in a pass of their own
rm -rf $OUT/prof_mfma
timeout -k 10 300 rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE --output-format csv -d $OUT/prof_mfma -o m -- python3 $R/bench.py --no-graph --steps 3 --warmup 1 --no-cpu-baseline --no-roofline --no-secondary > $OUT/prof_mfma.log 2>&1
rm -f $OUT/prof_mfma/*/*kernel_trace.csv $OUT/prof_mfma/*kernel_trace.csv
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_c3 -o s -- python3 $R/bench.py --workload c3 --full --no-cpu-baseline --no-roofline > $OUT/prof_c3.log 2>&1
rm -f $OUT/prof_c3/*/*kernel_trace.csv $OUT/prof_c3/*kernel_trace.csv
cd $R
timeout -k 10 400 python3 bench.py --full > $OUT/bench_official.log 2>&1
timeout -k 10 300 python3 bench.py --full --dtype f32 --no-cpu-baseline > $OUT/bench_f32.log 2>&1
timeout -k 10 400 python3 bench.py --full --workload c3 > $OUT/bench_c3.log 2>&1
timeout -k 10 300 python3 bench.py --full --workload c5 --steps 3 --warmup 1 > $OUT/bench_c5.log 2>&1
for f in official f32 c3 c5; do grep "^{" $OUT/bench_$f.log | tail -1 | cut -c1-260; done
