#!/bin/bash
# rocprofv3 kernel stats + PMC bytes (profile_round.sh), MFMA busy (pmc_mfma.sh), then the fp32
# bench with extras, on one box.  usage (GPU box, repo root): bash tools/profile_all.sh <tag>
set -o pipefail
bash tools/profile_round.sh "$1" &&
  bash tools/pmc_mfma.sh "gpurun_out/$1/pmc_mfma" f32_fft &&
  out=$(dirname "$(ls -t */"$1"/DONE | head -n 1)") &&   # the directory profile_round.sh just wrote
  timeout -k 10 420 python bench.py --full > "$out/bench_full_fp32.json" 2> "$out/bench_fp32.err"
