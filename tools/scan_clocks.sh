# GPU box: where a wave of the group scan of 129-160 nt reads (work counters off) spends its cycles at bench size: the gather wait (from the issue of a step's gathers
# to its frame), the read loop, and the rest of hs_group, as shares of the wave cycles in hs_group.
# Build the diagnostic library first (build container): bash tools/build_variant.sh clocks -DBSX_SCAN_CLOCKS [-DHG_LEAN=0 for the loop of round 10]
# Only the C3 bench (--mode pe) reports.  usage: bash tools/scan_clocks.sh <out-dir> <tag> [variant name, default clocks]   ->  <out-dir>/<tag>_scan_clocks.txt
O=${1:?out-dir}; TAG=${2:-clocks}; V=${3:-clocks}
R=$(cd "$(dirname "$0")/.." && pwd); mkdir -p $O; O=$(cd $O && pwd); cd $R
export BSX_LIB=$R/bsmap_amd/libbsx_$V.so
timeout -k 10 600 python3 bench.py --mode pe --in-flight 1 --steps 2 --warmup 1 2> $O/${TAG}_scan_clocks.err > /dev/null || { echo "failed"; tail -3 $O/${TAG}_scan_clocks.err; exit 1; }
grep scanclocks $O/${TAG}_scan_clocks.err | tail -1 | tee $O/${TAG}_scan_clocks.txt   # (the counters add up over the run: the last line)
