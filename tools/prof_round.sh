#!/bin/bash
# Round profile: bench line (--full) + rocprofv3 kernel stats + the two HBM-traffic PMC passes (separate runs, kernel trace only).
#   bash tools/prof_round.sh r02_final [OUT]       (on the GPU box; everything is written under OUT, default prof_out/)
TAG=${1:-r02}; OUT=${2:-prof_out}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p $OUT
python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_stats -o stats -- python3 bench.py --steps 20 --warmup 3 --no-extra > $OUT/${TAG}_stats.log 2>&1
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/${TAG}_fetch -o fetch -- python3 bench.py --steps 3 --warmup 1 --no-extra > $OUT/${TAG}_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/${TAG}_write -o write -- python3 bench.py --steps 3 --warmup 1 --no-extra > $OUT/${TAG}_write.log 2>&1
ls -R $OUT/${TAG}_* | head -30
tail -c 3000 $OUT/${TAG}_bench.json
