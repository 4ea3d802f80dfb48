# Round-end style GPU check: the full -m gpu suite, smoke(), the full bench (line + detail file) and
# the 2-rank shared-GPU rehearsal of the multi-rank bench path.  usage: bash tools/gpu_round_check.sh rNN
# (logs and results go to $OUT, default bench_out/)
set -o pipefail
R=${1:-r05}
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/${R}_tests.log 2>&1 && \
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${R}_smoke.log 2>&1 && \
timeout -k 10 700 python bench.py --full --detail-out $OUT/${R}_bench_detail.json > $OUT/${R}_bench.json 2> $OUT/${R}_bench.err && \
timeout -k 10 600 python bench.py --full --gpus 2 --share-gpu --steps 3 --warmup 1 --cpu-budget 0 --no-fp16-compare \
    --detail-out $OUT/${R}_share2_detail.json > $OUT/${R}_share2.json 2> $OUT/${R}_share2.err
