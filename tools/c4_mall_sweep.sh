#!/bin/bash
# c4 bench at several ADMM_OPT_MALL_STREAMS values (chunk = 224 MiB / (28 B/px x n)).  usage: tools/c4_mall_sweep.sh TAG "1 2 4 6 8"
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"; export PYTHONUNBUFFERED=1
# results go to $OUT_DIR (default bench_out/)
TAG=$1; O=${OUT_DIR:-bench_out}; mkdir -p $O
for n in $2; do
  timeout -k 10 200 python bench.py --full --config c4 --steps 5 --warmup 2 --no-cpu-baseline --opt MALL_STREAMS=$n > $O/${TAG}_n$n.jsonl 2>/dev/null || exit $?
  python -c "import json,sys; d=json.loads(open(sys.argv[1]).readline()); print(sys.argv[2], d['value'], d['ms_per_step'], d['roofline']['schedule'])" $O/${TAG}_n$n.jsonl $n
done
