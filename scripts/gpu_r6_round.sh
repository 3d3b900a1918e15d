#!/bin/bash
# Round-6 evidence: bench line, per-config records with the CPU learn() of C3 / C4-shard run in full and the config-5 front door.
# Run on the GPU box from the repo root: bash scripts/gpu_r6_round.sh OUT_DIR   (the bench line and the configs log go to OUT_DIR;
# gpu_configs.py writes its per-config records where it always does)
set -u
o=${1:?usage: gpu_r6_round.sh OUT_DIR}
mkdir -p "$o"
python bench.py --full > "$o/r6_bench.json" 2> "$o/r6_bench.err"
tail -c 400 "$o/r6_bench.json"
python scripts/gpu_configs.py c1 c2 c3 c4 c5 c5d --round r6 --cpu-full --front-door > "$o/r6_configs.log" 2>&1
tail -12 "$o/r6_configs.log"
