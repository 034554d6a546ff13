# Round-end evidence: the full bench line + rocprofv3 kernel stats + PMC traffic
# for the hot kernel, all from the same binary.  Writes profile_out/${OUT:-final}/
# under the repository root (or under $PROFILE_ROOT).
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
D=${PROFILE_ROOT:-$R/profile_out}/${OUT:-final}
mkdir -p $D && cd $R
# every leg (--full): CPU pool, ragged, e2e, re-verify beside the headline
timeout -k 10 600 python bench.py --full --detail $D/bench_detail.json > $D/bench.json 2> $D/bench.err || { echo BENCH_FAIL; tail -30 $D/bench.err; exit 1; }
cat $D/bench.json
cd /tmp && export TMPDIR=/tmp
# the trace takes the headline and the ragged leg; the counter runs are plain ones (the headline's kernel only)
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $D/trace -o bench -- python3 $R/bench.py --steps 20 --warmup 10 --full --no-cpu-baseline --no-e2e --no-reverify --detail $D/trace_detail.json > $D/trace.log 2>&1 || { echo TRACE_FAIL; tail -20 $D/trace.log; exit 1; }
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $D/pmc_fetch -o fetch -- python3 $R/bench.py --steps 3 --warmup 0 --detail $D/pmc_fetch_detail.json > $D/pmc_fetch.log 2>&1 || { echo PMC_FAIL; tail -20 $D/pmc_fetch.log; exit 1; }
timeout -k 10 300 rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_WAVES SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_SALU --output-format csv -d $D/pmc_sq -o sq -- python3 $R/bench.py --steps 3 --warmup 0 --detail $D/pmc_sq_detail.json > $D/pmc_sq.log 2>&1 || { echo PMC_FAIL; tail -20 $D/pmc_sq.log; exit 1; }
grep -h sha1 $D/trace/bench_kernel_stats.csv
