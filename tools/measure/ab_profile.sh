#!/bin/bash
# Kernel stats and PMC traffic of the headline command for a list of library builds, every collection in a run of its own (PMC and
# tracing are never combined): [OUT=dir] tools/measure/ab_profile.sh NAME=path/to/libqoi_mi355x.so ...   ->  $OUT/NAME_{stats,pmc_*} (default build/prof)
# Each build is copied over qoi_amd/lib/libqoi_mi355x.so for its runs; the tree's own library is put back at the end.
set -u
cd "$(dirname "$0")/../.."; export PYTHONUNBUFFERED=1
R=$PWD; O=${OUT:-build/prof}; mkdir -p "$O"; O=$(cd "$O" && pwd)
LIB=qoi_amd/lib/libqoi_mi355x.so
KEEP=$(mktemp /tmp/libqoi_keep.XXXXXX); cp $LIB "$KEEP"
restore() { cp "$KEEP" $LIB; rm -f "$KEEP"; }
BENCH="python $R/bench.py --no-cpu --no-others --no-single --no-configs"
for arg in "$@"; do
  who=${arg%%=*}; lib=${arg#*=}
  [ "$lib" -ef $LIB ] || cp "$lib" $LIB
  (cd /tmp && timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/${who}_stats" -o trace -- $BENCH --steps 5 --warmup 2) > "$O/${who}_stats.log" 2>&1; rc=$?
  echo "$who stats rc=$rc"; [ $rc -ne 0 ] && { restore; exit $rc; }
  for set in FETCH_SIZE WRITE_SIZE; do
    (cd /tmp && timeout -k 10 240 rocprofv3 --kernel-trace --pmc $set --output-format csv -d "$O/${who}_pmc_$set" -o pmc -- $BENCH --steps 3 --warmup 1) > "$O/${who}_pmc_$set.log" 2>&1; rc=$?
    echo "$who $set rc=$rc"; [ $rc -ne 0 ] && { restore; exit $rc; }
  done
  cp "$KEEP" $LIB
done
restore
