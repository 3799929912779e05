#!/bin/bash
# usage: [OUT=<dir>] tools/bench_configs.sh <tag> <config> [<config> ...]   — one bench line per config (with its stage times) into
# <dir>/<tag>_<config>_<dtype>.json + a summary; <dir> defaults to bench_out/
TAG=$1; shift
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
for c in "$@"; do
  cfg=${c%%:*}; dt=fp32; [[ "$c" == *:bf16 ]] && dt=bf16
  timeout -k 10 300 python3 bench.py --full --config $cfg --dtype $dt --steps 10 --warmup 3 --no-cpu-baseline > "$OUT/${TAG}_${cfg}_${dt}.json" 2>"$OUT/${TAG}_${cfg}_${dt}.err" || { echo "$c failed"; tail -3 "$OUT/${TAG}_${cfg}_${dt}.err"; exit 1; }
  python3 - <<PY
import json
j = json.load(open("$OUT/${TAG}_${cfg}_${dt}.json"))
print("${cfg} ${dt}", round(j["ms_per_step"], 3), {k: round(v, 3) for k, v in j["stages_ms"].items()}, j.get("parity"))
PY
done
