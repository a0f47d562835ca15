# Round-end bench line + rocprofv3 kernel trace/stats of the same bench command (CSV).
set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${1:-$(mktemp -d)}  # where the bench line goes: the first argument, else a fresh temporary directory
timeout -k 10 300 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err || exit $?
cat $OUT/bench.json
cd /tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $GRAFT_REPO_ROOT/gpurun_out/prof -o run -- python3 $GRAFT_REPO_ROOT/bench.py --steps 5 --warmup 2 > $GRAFT_REPO_ROOT/gpurun_out/prof.log 2>&1 || exit $?
