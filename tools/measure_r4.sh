#!/bin/bash
# One GPU-box pass that produces the round-4 measurement set under gpurun_out/profiles/ (copied into profiles/ afterwards).
cd "$GRAFT_REPO_ROOT"; mkdir -p gpurun_out/profiles; P=gpurun_out/profiles
b() { python bench.py --full "$@" 2>/dev/null | tail -1; }
b > $P/r4_bench_lo.json
b --mode vl --no-cpu-baseline > $P/r4_bench_vl.json
b --dtype fp16 --no-cpu-baseline > $P/r4_bench_lo_fp16.json
b --res hi --no-cpu-baseline --steps 10 --warmup 3 > $P/r4_bench_hi_bf16.json
b --res hi --attn fp8 --no-cpu-baseline --steps 10 --warmup 3 > $P/r4_bench_hi_fp8.json
b --block l0hi --steps 20 --warmup 3 > $P/r4_block_l0hi_bf16.json
b --block l0hi --attn fp8 --steps 20 --warmup 3 > $P/r4_block_l0hi_fp8.json
for f in lo vl lo_fp16 hi_bf16 hi_fp8; do python -c "import json,sys; d=json.load(open('$P/r4_bench_$f.json')); print('$f', round(d['ms_per_step'],3), 'ms', round(d['config']['step_mfma_frac_of_peak'],4), d['roofline']['kernel'] if d['roofline'] else '', round(d['roofline']['frac'],4) if d['roofline'] else '')"; done
for f in bf16 fp8; do python -c "import json; d=json.load(open('$P/r4_block_l0hi_$f.json')); print('block $f', round(d['ms_per_step'],3), 'ms frac', round(d['roofline']['frac'],4))"; done
bash tools/profile_round.sh r4_vgl_lo_bf16 lo 2>&1 | tail -30
