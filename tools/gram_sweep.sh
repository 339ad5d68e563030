#!/bin/bash
# Sweep of IRM_GRAM_BLOCKS on the headline command (run from the repo root on an MI355X): per setting the Gram rows
# of the kernel table and ms_per_step.   tools/gram_sweep.sh [OUT_DIR]   (default: a fresh temporary directory)
OUT=${1:-$(mktemp -d)}; mkdir -p $OUT
for tb in 1024 2048 3072 4096 6144; do echo TB=$tb; IRM_GRAM_BLOCKS=$tb python bench.py --full --no-cpu-baseline --steps 4 --detail $OUT/gd_$tb.json > $OUT/g_$tb.json 2>/dev/null; python tools/show_detail.py $OUT/gd_$tb.json 4 60 | grep "gram"; python -c "import json;print(json.load(open('$OUT/g_$tb.json'))['ms_per_step'])"; done
