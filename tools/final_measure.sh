#!/bin/bash
# Round-end measurement set (GPU box): full bench line, bs 8 (BASELINE configs[1]), MoCE-IR, AdaIR, kernel tables, into OUT_DIR.
OUT=${1:?usage: tools/final_measure.sh OUT_DIR}
mkdir -p "$OUT"
python bench.py --full --profile-json "$OUT/kernel_table_bs32.json" > "$OUT/bench_bs32.log" 2>&1
python bench.py --full --batch 8 --no-cpu-baseline > "$OUT/bench_bs8.log" 2>&1
python bench.py --full --model moce --no-cpu-baseline --profile-json "$OUT/moce_kernel_table.json" > "$OUT/bench_moce.log" 2>&1
python bench.py --full --model adair --batch 8 --no-cpu-baseline > "$OUT/bench_adair.log" 2>&1
for f in bs32 bs8 moce adair; do tail -c 600 "$OUT/bench_$f.log" | head -c 300; echo; done
