#!/bin/bash
# rocprofv3 per-kernel summary of the headline bench command: tools/kernel_stats.sh OUTDIR
R=$(cd "$(dirname "$0")/.." && pwd)
O=$(realpath -m "${1:?usage: tools/kernel_stats.sh OUTDIR}")
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/rp -- python3 $R/bench.py --full --steps 50 --warmup 5 --no-cpu-baseline > $O/rp.json 2> $O/rp.log
head -7 $(find $O/rp -name "*kernel_stats.csv" | head -1) | cut -c1-150
