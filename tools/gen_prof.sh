# rocprofv3 kernel stats of the headline bench (generator forward, B=16): bash tools/gen_prof.sh <tag>
# (written to $PROF_OUT, default prof_out/ in the repository root; the summary line reads the --full record's roofline)
TAG=${1:-r02_gen}
ROOT=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${PROF_OUT:-$ROOT/prof_out}
export PROF_OUT=$OUT
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/$TAG
rocprofv3 --kernel-trace --stats -d $OUT/$TAG -o prof -- python $ROOT/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-exact-fp32 --train-steps 0 --no-stream > $OUT/$TAG.json 2> $OUT/$TAG.err
DB=$(find $OUT/$TAG -name "*results.db" | head -1)
python $ROOT/tools/rocpd_summary.py stats $DB $OUT/${TAG}_kernel_stats.md | head -40
rm -rf $OUT/$TAG
python -c "import json; d=json.load(open('$OUT/$TAG.json')); print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline']['avg_launch_us'])"
