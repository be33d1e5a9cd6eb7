# A/B two full library builds on one box, interleaved rounds: tools/lib_ab.sh <pathA> <pathB> ...  ("default" = the in-tree library)
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
L=$(mktemp)
for r in 1 2 3; do for v in "$@"; do
  if [ "$v" = default ]; then unset MST_ENGINE_LIB; else export MST_ENGINE_LIB=$PWD/$v; fi
  timeout -k 10 300 python bench.py --steps 2 --warmup 1 --full --no-cpu-baseline --no-boundary > $L 2>&1
  tail -1 $L | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('$v', d['value'], {k:v['avg_launch_us'] for k,v in d['roofline']['families'].items() if v['avg_launch_us']>10})"
done; done
