#!/bin/bash
# Two-stream bench at several batch sizes / stream counts (10 steps, no CPU legs).
# usage: tools/sweep_batch2.sh "B:S ..."  -> $out/sweep/<B>_<S>.json
set -e
out=${DVO_OUT:-out}; mkdir -p "$out"  # results go under $DVO_OUT (default out/)
mkdir -p $out/sweep
for bs in $1; do
  b=${bs%%:*}; s=${bs##*:}
  timeout -k 10 200 python -u bench.py --full --cpu-seconds 0 --config-legs none --no-ref-equivalent --no-host-fed --tail-world 0 --dropin-seconds 0 --steps 10 --warmup 2 --batch $b --streams $s > $out/sweep/${b}_${s}.json 2> $out/sweep/${b}_${s}.err
  echo "$b $s $(python3 -c "import json; d=json.load(open('$out/sweep/${b}_${s}.json')); print(d['value'], d['ms_per_step'])")"
done
