# Round-4 measurement record (run on the GPU box through gpurun; writes gpurun_out/final4/, copied to profiles/r04/h_*):
# GPU tests, smoke, the default bench line, rocprofv3 kernel stats of the SAME command, HBM-side traffic of every
# configuration's roofline kernel (FETCH_SIZE and WRITE_SIZE in SEPARATE --pmc passes, MI355X_MICROARCH.md "rocprofv3 PMC
# slots"), SQ counters of the IPDnet2 scan kernel.   Usage: bash tools/gpu_final_r04.sh [quick]
R=$GRAFT_REPO_ROOT; O=$R/gpurun_out/final4; mkdir -p $O; cd $R
if [ "$1" != "quick" ]; then
  timeout 1500 python -m pytest tests -q -m gpu -p no:cacheprovider 2>&1 | tail -4 > $O/pytest.log
  timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1
fi
timeout 600 python bench.py --full --steps 20 --warmup 5 > $O/bench_default.json 2> $O/bench.err
export TMPDIR=/tmp; cd /tmp
timeout 500 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o r1 -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --ab-steps 0 > $O/prof.log 2>&1
cp $(ls $O/prof/*kernel_stats.csv | head -1) $O/kernel_stats_bench_default_steps3.csv; rm -rf $O/prof
for cfg in 2 3 4 5; do
  for c in FETCH_SIZE WRITE_SIZE; do
    timeout 300 rocprofv3 --pmc $c --output-format csv -d $O/pmc_$c -o p -- python $R/bench.py --config $cfg --steps 1 --warmup 1 --no-cpu-baseline --other-configs "" --ab-steps 0 > $O/pmc_${cfg}_$c.log 2>&1
    python $R/tools/pmc_summary.py $(ls $O/pmc_$c/*counter_collection.csv | head -1) "lstm_static3|lstm_bf16c_kernel<256|lstm_bwd2_kernel<256|sn_mamba_scan" > $O/pmc_c${cfg}_$c.json; rm -rf $O/pmc_$c
  done
done
timeout 300 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_INSTS_VALU GRBM_GUI_ACTIVE --output-format csv -d $O/pmc5 -o p -- python $R/bench.py --config 5 --steps 1 --warmup 1 --no-cpu-baseline --other-configs "" > $O/pmc5.log 2>&1
python $R/tools/pmc_summary.py $(ls $O/pmc5/*counter_collection.csv | head -1) "sn_mamba_scan" > $O/pmc_c5_sq_scan.json; rm -rf $O/pmc5
cd $R; python tools/hbm_traffic_r04.py $O > $O/hbm_traffic.json
cat $O/pytest.log 2>/dev/null; tail -1 $O/smoke.log 2>/dev/null; cut -c1-300 $O/bench_default.json; tail -2 $O/bench.err
head -12 $O/kernel_stats_bench_default_steps3.csv | cut -c1-170; cat $O/hbm_traffic.json; cat $O/pmc_c5_sq_scan.json
