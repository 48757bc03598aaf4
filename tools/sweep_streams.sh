#!/bin/bash
# Default-bench frames/s over (streams, batch) shapes (no CPU / drop-in legs, no stage events).
# usage: tools/sweep_streams.sh "CFG1" "CFG2" ...   (each CFG a string of bench.py flags)
set -e
out=${DVO_OUT:-out}; mkdir -p "$out"  # results go under $DVO_OUT (default out/)
mkdir -p $out/sweep
for cfg in "$@"; do
  tag=$(echo $cfg | tr -d ' -')
  timeout -k 10 200 python -u bench.py --full --cpu-seconds 0 --config-legs none --no-ref-equivalent --no-host-fed --tail-world 0 --dropin-seconds 0 --no-profile --steps 8 $cfg > $out/sweep/$tag.log 2>&1
  echo "$cfg $(tail -1 $out/sweep/$tag.log | python3 -c 'import json,sys; d=json.loads(sys.stdin.read()); print(d["value"], d["ms_per_step"])')"
done
