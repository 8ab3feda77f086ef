# rocprofv3 kernel-trace + stats summaries of bench workloads (short runs): MODELS="adain wct sanet".
# Usage: OUT_DIR=<folder> bash tools/prof_stats.sh
set -e
R=$GRAFT_REPO_ROOT
O=${OUT_DIR:?set OUT_DIR to the folder the traces and logs go to}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
for m in ${MODELS:-adain wct sanet}; do
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$m -o $m -- python3 $R/bench.py --full --model $m --steps 3 --warmup 1 --no-cpu-baseline > $O/prof_$m.log 2>&1
done
