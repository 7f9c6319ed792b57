#!/bin/bash
# One GPU-box pass producing the round's measurement record (copied to profiles/ by
# tools/summarize_profiles.py): the bench JSON line with every leg (bench.py --full), the rocprofv3
# --kernel-trace --stats summary of the same bench command, and the two HBM-traffic PMC passes
# (FETCH_SIZE and WRITE_SIZE cannot share a pass on gfx950). Every GPU step has its own time limit;
# steps are chained with &&.   Usage: tools/profile_round.sh [out-dir]   (default prof_out)
set -o pipefail
O=${1:-prof_out}
mkdir -p "$O"
export TMPDIR=/tmp
B="python bench.py --full --no-extras --no-cpu --steps 50"
timeout -k 10 400 python bench.py --full > "$O/bench.json" 2> "$O/bench.err" &&
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/trace" -o trace -- \
    $B > "$O/trace.log" 2>&1 &&
timeout -k 10 400 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d "$O/fetch" -o fetch -- \
    $B > "$O/fetch.log" 2>&1 &&
timeout -k 10 400 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d "$O/write" -o write -- \
    $B > "$O/write.log" 2>&1
rc=$?
echo "profile rc=$rc"
exit $rc
