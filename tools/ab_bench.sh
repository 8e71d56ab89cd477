#!/bin/bash
# A/B on ONE box (boxes of the pool differ by 8 % on the search kernel): alternates bench.py between bwt-merge_amd/_variants/base.so
# (tools/build_variant.sh base "" on the commit to compare with) and the library in the tree.  Usage: bash tools/ab_bench.sh [kernel ...]
# AB_BENCH_ARGS: extra bench.py arguments of both sides (another workload than config 2).  Every run has its own time limit, and the first run that fails ends the script.
keys=${@:-frontier_step}; line=$(mktemp); trap 'rm -f "$line"' EXIT
for v in base cur base cur base cur; do
  if [ $v = base ]; then export BWTM_LIB=$PWD/bwt-merge_amd/_variants/base.so; else unset BWTM_LIB; fi
  timeout -k 10 ${AB_BENCH_TIMEOUT:-600} python bench.py --full --steps 10 --warmup 2 --no-host --no-cpu-baseline --no-verify --target off $AB_BENCH_ARGS 2>/dev/null > $line.all
  rc=$?; if [ $rc -ne 0 ]; then echo "$v: bench.py ended with status $rc; stopping"; rm -f $line.all; exit $rc; fi
  tail -1 $line.all > $line; rm -f $line.all
  python3 - $line $v $keys <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read()); k = d["kernel_ms_per_step"]
print(sys.argv[2], d["ms_per_step"], {x: k.get(x) for x in sys.argv[3:]})
PY
done
