#!/bin/bash
# bench.py on the headline (--full: with the CPU baseline) and on the other BASELINE configurations; one JSON line each.
# Usage: tools/bench_all.sh <tag> [out_dir]   -> <out_dir>/<tag>_bench_n1.json, <out_dir>/<tag>_bench_configs.jsonl
# (out_dir defaults to bench_out/, which git ignores)
set -e
tag=$1
out=${2:-bench_out}
mkdir -p "$out"
python bench.py --full > "$out/${tag}_bench_n1.json" 2> "$out/${tag}_bench_n1.err"
: > "$out/${tag}_bench_configs.jsonl"
python bench.py --scene cornell --nx 600 --ny 600 --ns 1000 >> "$out/${tag}_bench_configs.jsonl" 2>> "$out/${tag}_bench_n1.err"
python bench.py --scene cornell_smoke --nx 600 --ny 600 --ns 1000 >> "$out/${tag}_bench_configs.jsonl" 2>> "$out/${tag}_bench_n1.err"
python bench.py --scene final --nx 800 --ny 800 --ns 200 >> "$out/${tag}_bench_configs.jsonl" 2>> "$out/${tag}_bench_n1.err"
python bench.py --scene book1 --nx 1200 --ny 800 --ns 100 >> "$out/${tag}_bench_configs.jsonl" 2>> "$out/${tag}_bench_n1.err"
python bench.py --nx 1920 --ny 1080 --ns 500 >> "$out/${tag}_bench_configs.jsonl" 2>> "$out/${tag}_bench_n1.err"
