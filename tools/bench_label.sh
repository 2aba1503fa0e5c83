#!/bin/bash
# make_dataset --rng philox: --label host against --label native, alternating, ROUNDS rounds at each of
# the two points (M = 8 at 3.0 dB, M = 4 at 2.5 dB).  Every step is one process under its own time
# limit; the first step that fails ends the script.  One JSON line per step (tools/bench_label.py).
#   tools/bench_label.sh [frames] [rounds] [out file]
FRAMES=${1:-4194304}
ROUNDS=${2:-5}
OUT=${3:-_out/label_bench.jsonl}
LIMIT=${LIMIT:-600}
cd "$(dirname "$0")/.." || exit 1
mkdir -p "$(dirname "$OUT")"
: > "$OUT"
for r in $(seq 1 "$ROUNDS"); do
    if [ -n "$BUDGET" ] && [ "$SECONDS" -gt "$BUDGET" ]; then  # (no new round past BUDGET seconds)
        echo "stopping before round $r: $SECONDS s used" >&2
        break
    fi
    for point in "8 3.0" "4 2.5"; do
        set -- $point
        for label in host native; do
            timeout -k 10 "$LIMIT" python tools/bench_label.py --label "$label" --M "$1" --snr_db "$2" \
                --frames "$FRAMES" --batch 65536 | tee -a "$OUT"
            rc=${PIPESTATUS[0]}
            if [ "$rc" -ne 0 ]; then
                echo "step failed (rc=$rc): round $r, M=$1, $2 dB, $label" >&2
                exit "$rc"
            fi
        done
    done
done
