# Everything profiles/ holds for one tag, in one GPU call:  bash tools/round_profiles.sh r03z
# (written to $PROF_OUT, default prof_out/ in the repository root)
#   <tag>_bench.json                       python bench.py --full (every leg of the benchmark)
#   <tag>_gen_kernel_stats.md              rocprofv3 --kernel-trace --stats of the generator leg
#   <tag>_pmc_{mfma,wait,fetch,write}.md   PMC passes (separate runs, --pmc with --kernel-trace only)
#   <tag>_hbm_per_kernel.md                HBM bytes / achieved TB/s per kernel from the fetch / write passes
#   <tag>_train_{bf16x3,bf16}_kernel_stats.md   rocprofv3 stats of the train step in both arithmetic modes
TAG=${1:-r03z}
ROOT=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${PROF_OUT:-$ROOT/prof_out}
export PROF_OUT=$OUT
mkdir -p $OUT
cd $ROOT
python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
bash tools/gen_prof.sh ${TAG}_gen > $OUT/${TAG}_gen_prof.log 2>&1
mv $OUT/${TAG}_gen_kernel_stats.md $OUT/${TAG}_gen_kernel_stats.md 2>/dev/null
bash tools/pmc_prof.sh ${TAG} > $OUT/${TAG}_pmc.log 2>&1
python tools/hbm_table.py $OUT/${TAG}_pmc_fetch.json $OUT/${TAG}_pmc_write.json $OUT/${TAG}_gen_gen_kernel_stats.md $OUT/${TAG}_hbm_per_kernel.md 30 > /dev/null 2>&1 || \
python tools/hbm_table.py $OUT/${TAG}_pmc_fetch.json $OUT/${TAG}_pmc_write.json $OUT/${TAG}_gen_kernel_stats.md $OUT/${TAG}_hbm_per_kernel.md 30 > /dev/null 2>&1
cd /tmp && export TMPDIR=/tmp
for MODE in bf16x3 bf16; do
  rm -rf $OUT/${TAG}_tr_$MODE
  APAMD_PRECISION=$MODE rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_tr_$MODE -o prof -- python $ROOT/tools/train_bench.py 16 5 > $OUT/${TAG}_train_$MODE.log 2>&1
  DB=$(find $OUT/${TAG}_tr_$MODE -name "*results.db" | head -1)
  python $ROOT/tools/rocpd_summary.py stats $DB $OUT/${TAG}_train_${MODE}_kernel_stats.md > /dev/null
  rm -rf $OUT/${TAG}_tr_$MODE
  tail -2 $OUT/${TAG}_train_$MODE.log
done
ls $OUT | grep "^${TAG}"
