#!/bin/bash
# Dev (round 6): the bench's 25-step val Dice (bench.py --full) across trainer seeds on ONE tree (bs320, 20+5
# steps, the same protocol as BENCH_r0N.json) -> ${OUT:-bench_out}/dice_spread/seed_<s>.json: how far
# summation-order-free run-to-run differences (a different init / data order) move that number.
set -e
out=${OUT:-bench_out}/dice_spread
mkdir -p $out
for sd in ${SEEDS:-1 2 3 4}; do
  timeout -k 10 400 python -u bench.py --full --seed $sd > $out/seed_$sd.json 2> $out/seed_$sd.err
done
