set -e
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-profile_out}  # where the results go
mkdir -p "$OUT"
bash profiles/run_profile.sh r02_jacobi > $OUT/prof_r02_jacobi.log 2>&1
python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $OUT/bench_steps20.json 2>/dev/null
python bench.py --full --uvt --steps 2000 --warmup 200 --no-cpu-baseline > $OUT/bench_uvt.json 2>/dev/null
: > $OUT/bench_other.jsonl
for w in slj_256 ses_1024 spol_1024 spol_4096 spol_16384 spolprod_1024 spolprod_4096; do
  python bench.py --full --workload $w --steps 1500 --warmup 150 --no-cpu-baseline 2>/dev/null | grep "^{" >> $OUT/bench_other.jsonl
  echo done $w
done
bash profiles/run_profile.sh r02_gs --workload spolprod_4096 > $OUT/prof_r02_gs.log 2>&1
python bench.py --full --workload spolprod_4096 --uvt --steps 1000 --warmup 100 --no-cpu-baseline > $OUT/bench_gs_uvt.json 2>/dev/null
echo ALL DONE
