#!/bin/bash
# same-box A/B of several builds on the cooling block (python bench.py --cooling-only: the production cooling kernel on a multiphase medium), three
# interleaved rounds:   bash profiles/tools/ab_trees_cooling.sh <tree> ...   — each <tree> a checkout with its library and oracle built (a build
# whose C-ABI differs cannot be swapped in through QK_LIB_PATH, so whole trees are compared).  Name the parent's tree twice (a copy under a second
# name): the difference between its two series is the run-to-run spread on this box, the margin inside which the result must lie.  A run that
# fails ends the job.  The table goes to standard output.
tmp=$(mktemp -d) || exit 1
trap 'rm -rf "$tmp"' EXIT
for rep in 1 2 3; do
  for tree in "$@"; do
    (cd "$tree" && timeout -k 10 150 python bench.py --cooling-only 2>$tmp/err.txt > $tmp/line.json) || { echo "bench.py failed: tree=$tree"; tail -5 $tmp/err.txt; exit 1; }
    python -c "
import json
d = json.loads(open('$tmp/line.json').readline())['cooling128']
keep = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in d.items() if isinstance(v, (int, float))}
print('tree=$tree rep=$rep', json.dumps(keep))" || exit 1
  done
done
