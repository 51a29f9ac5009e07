# GPU box: mean 32-nt words per (read, 64-candidate chunk) evaluation of the group scan's exiting form (same_exit) at bench size.
# Build the diagnostic library first (build container): bash tools/build_variant.sh words -DBSX_SCAN_WORDS
# Only reads of 129-160 nt take that form, so only the C3 bench (--mode pe) reports.
# usage: bash tools/scan_words.sh <out-dir> <tag>   ->  <out-dir>/<tag>_scan_words.txt
O=${1:?out-dir}; TAG=${2:-words}; MODES=pe
R=$(cd "$(dirname "$0")/.." && pwd); mkdir -p $O; O=$(cd $O && pwd); cd $R
export BSX_LIB=$R/bsmap_amd/libbsx_words.so
for m in $MODES; do
  timeout -k 10 600 python3 bench.py --mode $m --in-flight 1 --steps 2 --warmup 1 2> $O/${TAG}_scan_words_$m.err > /dev/null || { echo "$m failed"; tail -3 $O/${TAG}_scan_words_$m.err; exit 1; }
  grep scanwords $O/${TAG}_scan_words_$m.err | awk -v m=$m '{ last[$2] = $0 } END { for (k in last) print m, last[k] }'   # (the counters add up over the run: the last line of a class)
done | tee $O/${TAG}_scan_words.txt
