# End-of-round profiles (GPU box): kernel stats of the full bench (`bench.py --full`), PMC passes of the sketch kernel,
# counters of the merge kernel at C4.  Text summaries go to prof_out/ under the repository (override with OUT=...); the
# rocpd databases stay under $TMPDIR.
set -e
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$REPO/prof_out}; mkdir -p $OUT
W=${TMPDIR:-/tmp}/prof
S=$REPO/profiles/summarize.py
B="python $REPO/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-compare"
cd ${TMPDIR:-/tmp}
rocprofv3 --kernel-trace --stats -d $W/stats -o bench -- python $REPO/bench.py --full > $OUT/prof_bench_stdout.txt 2> $W.stats.log || tail -3 $W.stats.log
python $S $(find $W/stats -name "*.db" | head -1) > $OUT/r01_end_kernel_stats.txt
for C in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $C -d $W/$C -o bench -- $B > /dev/null 2> $W.$C.log || tail -3 $W.$C.log
done
rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_WAVES SQ_INSTS_SALU SQ_WAIT_INST_ANY -d $W/SQ -o bench -- $B > /dev/null 2> $W.SQ.log || tail -3 $W.SQ.log
python $S $(find $W/FETCH_SIZE -name "*.db" | head -1) $(find $W/WRITE_SIZE -name "*.db" | head -1) $(find $W/SQ -name "*.db" | head -1) > $OUT/r01_end_pmc.txt
rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_ANY SQ_WAVE_CYCLES GRBM_GUI_ACTIVE -d $W/CMP -o cmp -- python $REPO/tools/bench_compare.py c4 > $OUT/prof_cmp_stdout.txt 2> $W.CMP.log || tail -3 $W.CMP.log
python $S $(find $W/CMP -name "*.db" | head -1) > $OUT/r01_end_compare_pmc.txt
tail -1 $OUT/prof_bench_stdout.txt | cut -c1-300
head -8 $OUT/r01_end_kernel_stats.txt
grep -A12 "counter" $OUT/r01_end_compare_pmc.txt | grep compare_tile
