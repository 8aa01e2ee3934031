# Bench lines for every BASELINE config that fits one GPU (configs[1..3] + the maze/heist mix).
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}  # where the logs and JSON lines go
export TMPDIR=/tmp
mkdir -p $OUT/bench
S=${STEPS:-200}; W=${WARMUP:-50}
timeout -k 10 300 python3 bench.py --full --steps $S --warmup $W > $OUT/bench/coinrun.json 2> $OUT/bench/coinrun.err && \
timeout -k 10 300 python3 bench.py --full --env-name bigfish --steps $S --warmup $W --no-cpu-baseline > $OUT/bench/bigfish.json 2> $OUT/bench/bigfish.err && \
timeout -k 10 300 python3 bench.py --full --env-name maze --num-envs 32768 --steps $S --warmup $W --no-cpu-baseline > $OUT/bench/maze.json 2> $OUT/bench/maze.err && \
timeout -k 10 300 python3 bench.py --full --env-name heist --num-envs 32768 --steps $S --warmup $W --no-cpu-baseline > $OUT/bench/heist.json 2> $OUT/bench/heist.err && \
timeout -k 10 300 python3 bench.py --full --env-name maze,heist --num-envs 65536 --steps $S --warmup $W --no-cpu-baseline > $OUT/bench/maze_heist.json 2> $OUT/bench/maze_heist.err
rc=$?
for f in $OUT/bench/*.json; do echo "== $f"; python3 -c "import json,sys; d=json.load(open('$f')); print(d['value'], d['config']['env_name'], d['roofline']['kernel_ms'])" ; done
tail -2 $OUT/bench/*.err
exit $rc
