#!/bin/bash
# GPU box, repo root: the whole -m gpu suite (no -x, full log), smoke(), then the bench in its standard form with --full.
#   bash tools/gpucheck.sh [tag] [pytest -k expression]        logs go to $GPUCHECK_OUT (default: check_out/)
TAG=${1:-check}; K=${2:-}; O=${GPUCHECK_OUT:-check_out}
mkdir -p $O
if [ -n "$K" ]; then python3 -m pytest tests -q -m gpu -k "$K" > $O/${TAG}_pytest.log 2>&1
else python3 -m pytest tests -q -m gpu > $O/${TAG}_pytest.log 2>&1; fi
tail -n 30 $O/${TAG}_pytest.log | cut -c1-400
if [ -z "$K" ]; then
python3 -c "import __graft_entry__ as g; g.smoke(); print('smoke OK')" 2>&1 | tail -2
python3 bench.py --gpus 1 --steps 20 --warmup 5 --full --detail $O/${TAG}_bench_detail.json > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err
wc -c $O/${TAG}_bench.json; python3 tools/bench_summary.py $O/${TAG}_bench.json
fi
