#!/bin/bash
# same-box A/B of several library builds on BOTH forms of the RK2 average — the default bench.py line (--rk2-mode carry) and --rk2-mode exact (the form
# `rk2_other_mode` times) —, three interleaved rounds:   bash profiles/tools/ab_libs_modes.sh <lib.so> ...   (QK_LIB_PATH)
# Name the parent's build twice (e.g. a copy under a second name): the difference between its two series is the run-to-run spread on this box,
# the margin inside which the result must lie.  A run that fails ends the job.  The table goes to standard output.
cd "$(dirname "$0")/../.." || exit 1
tmp=$(mktemp -d) || exit 1
trap 'rm -rf "$tmp"' EXIT
out=$tmp/ab_libs_modes.txt
: > $out
for rep in 1 2 3; do
  for mode in carry exact; do
    for lib in "$@"; do
      QK_LIB_PATH=$PWD/$lib timeout -k 10 120 python bench.py --gpus 1 --full --rk2-mode $mode --steps 20 --warmup 3 --no-cpu-baseline --no-secondary 2>/dev/null > $tmp/ab_line.json || { echo "bench.py failed: lib=$lib mode=$mode"; exit 1; }
      python -c "
import json
d=json.loads(open('$tmp/ab_line.json').readline())
k={a:round(b,4) for a,b in d.get('roofline', {}).get('all_kernels_ms_per_launch',{}).items() if a.startswith('k_')}
print('mode=$mode lib=$(basename $lib) rep=$rep value=%.1f ms_per_step=%.3f kernels=%s' % (d['value'], d['ms_per_step'], json.dumps(k)))" >> $out || exit 1
    done
  done
done
cat $out
