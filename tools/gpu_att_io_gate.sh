#!/bin/bash
# What the access SHAPE of the attention kernel's two ends is worth (the diagnostic library's TT_ATT_IO, read per launch):
#   0 = 8-byte context stores, a lane per row (the kernel before whole-row stores)   1 = whole-row stores through LDS (ships)
#   4 = stand-in: stores in the whole-row shape, registers as they stand             8 = stand-in: Q loads in the whole-row shape
#   12 = both stand-ins                                                              (4, 8, 12: wrong results by design)
# The variants alternate inside ONE process, three rounds of 20 launches each (after 3 of their own; 200 launches warm the process first); then 0 against 1 at the
# five lengths of EXPERIMENTS.md's attention tables.  Needs tools/att_bench_diag and libtt_hip_diag.so (make DIAG=1) built.
cd "$(dirname "$0")/.." || exit 1
set -e
echo "== gate: 1600 x 292, four waves, TT_ATT_IO = 0 4 8 12 1"
timeout -k 10 120 tools/att_bench_diag 1600 292 20 3 0,4,8,12,1
for len in 130 200 292 420 512; do
    echo "== before / after: 1600 x $len, TT_ATT_IO = 0 1"
    timeout -k 10 120 tools/att_bench_diag 1600 $len 20 3 0,1
done
