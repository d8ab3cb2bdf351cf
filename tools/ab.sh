#!/bin/bash
# A/B timing of kernel variants on the GPU box: tools/ab.sh [-c CONFIG] [-r ROUNDS] [-p] name...
# "base" = the product library, any other name = dd2360-raytracing_amd/variants/lib_<name>.so (built by hand with -D switches);
# a name with a slash = another checkout of the project, built (its own bench.py, binding and library: a parent commit whose
# library lacks entry points that this tree's binding asks for).
# The variants are timed in ROUNDS interleaved passes (clock / thermal drift hits all alike); prints per variant the
# median and minimum kernel time and the median step time.  -p also runs the GPU parity suite against the LAST variant.
# -s: time the budget selection instead (tools/adaptive_budget_study.py --select, which bench.py never runs): one table per variant,
# with a checksum of the chosen sets (e.g. tools/ab.sh -s base probe after tools/mkvariant.sh probe -DSWITCH).
cfg=c3; parity=0; rounds=3; selection=0
while getopts "c:pr:s" o; do case $o in c) cfg=$OPTARG;; p) parity=1;; r) rounds=$OPTARG;; s) selection=1;; esac; done
shift $((OPTIND - 1))
root=$(cd "$(dirname "$0")/.." && pwd)
if [ $selection = 1 ]; then
  for v in "$@"; do
    if [ "$v" = base ]; then unset RT_AMD_LIB; else export RT_AMD_LIB=$root/dd2360-raytracing_amd/variants/lib_$v.so; fi
    timeout -k 10 180 python "$root/tools/adaptive_budget_study.py" --select || { echo "$v FAILED"; exit 1; }
  done
  exit 0
fi
tmp=$(mktemp)
for ((k = 0; k < rounds; k++)); do
  for v in "$@"; do
    tree=$root
    case "$v" in
      base) unset RT_AMD_LIB;;
      */*) unset RT_AMD_LIB; tree=$(cd "$v" && pwd);;
      *) export RT_AMD_LIB=$root/dd2360-raytracing_amd/variants/lib_$v.so;;
    esac
    out=$(timeout -k 10 180 python "$tree/bench.py" --config "$cfg" --steps 8 --no-cpu-baseline --no-pmc 2>/dev/null) || { echo "$v FAILED"; exit 1; }
    echo "$out" | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$v', d['ms_per_step'], d['roofline']['kernel_ms'])" >> $tmp
  done
done
python - $tmp "$@" <<'PY'
import sys, statistics as st
rows = [l.split() for l in open(sys.argv[1])]
for v in dict.fromkeys(sys.argv[2:]):
    step = [float(r[1]) for r in rows if r[0] == v]; ker = [float(r[2]) for r in rows if r[0] == v]
    print("%-10s kernel median %7.3f min %7.3f ms   step median %7.3f ms   (%d runs)" % (v, st.median(ker), min(ker), st.median(step), len(ker)))
PY
rm -f $tmp
if [ $parity = 1 ]; then timeout -k 10 400 python -m pytest "$root/tests/test_gpu_parity.py" -x -q 2>&1 | tail -3; fi
