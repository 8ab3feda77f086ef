# A/B of prebuilt library variants (var/<name>/librpst.so) on the plain-residual 1x1 conv that is
# the yardstick of the SE block's gated conv (tools/bench_se.py --residual-only), interleaved by
# process, two rounds. Usage: LIBS="parent new" bash tools/ab_se.sh <tag> [bench_se args]
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
O=${OUT_DIR:-$R/profiles/se_attention}/${1:-ab_se}
shift
mkdir -p $O
cd $R
for rep in 1 2; do
  for v in $LIBS; do
    RPST_LIB=$R/var/$v/librpst.so timeout -k 10 300 python tools/bench_se.py --residual-only "$@" > $O/residual_${v}_$rep.log 2>&1 || { tail $O/residual_${v}_$rep.log; exit 1; }
    echo "$v rep $rep: $(grep -o '"shape": \[[0-9]*, [^}]*"ms_max": [0-9.]*' $O/residual_${v}_$rep.log | tr '\n' ' ')"
  done
done
