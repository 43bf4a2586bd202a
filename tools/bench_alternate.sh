#!/bin/bash
# bench.py alternating between this tree and a built checkout of another commit (usually the parent), the order swapped from
# round to round: one JSON line per run.
#   tools/bench_alternate.sh <other tree, built> <out.jsonl> [rounds = 4]
# Each run is its own process under its own time limit; the first run that fails ends the script.
OTHER=${1:?the other tree}; OUT=${2:?the output file}; ROUNDS=${3:-4}
HERE=$(cd "$(dirname "$0")/.." && pwd)
OPTS="--gpus 1 --steps 200 --warmup 3 --no-cpu-baseline --no-other-configs --no-host-pipeline --no-single-frame --no-check"
mkdir -p "$(dirname "$OUT")"; : > "$OUT"
run() {  # tree name, directory, round, position in the round
  line=$(cd "$2" && timeout -k 10 240 python bench.py $OPTS 2>/dev/null | tail -1) || return 1
  python - "$1" "$3" "$4" "$line" "$OPTS" <<'PY' >> "$OUT" || return 1
import json, sys
r = json.loads(sys.argv[4])
print(json.dumps({"what": "bench.py " + sys.argv[5], "tree": sys.argv[1], "round": int(sys.argv[2]), "position_in_round": int(sys.argv[3]),
                  "frames_per_s": round(r["value"], 1), "ms_per_step": round(r["ms_per_step"], 5)}))
PY
  tail -1 "$OUT"
}
for round in $(seq 1 "$ROUNDS"); do
  if [ $((round % 2)) -eq 1 ]; then
    run parent "$OTHER" "$round" 1 || exit 1; run new "$HERE" "$round" 2 || exit 1
  else
    run new "$HERE" "$round" 1 || exit 1; run parent "$OTHER" "$round" 2 || exit 1
  fi
done
